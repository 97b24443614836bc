"""The host side of the weighted cross-entropy that needs no GPU: the --class_weights option, the "balanced" rule, the command line."""
import numpy as np
import pytest

from road_segmentation_unet_amd.cli import parse_options
from road_segmentation_unet_amd.model import EXTRA_FLAG_DEFS, Options, balanced_class_weights, parse_class_weights


def test_class_weights_option_parses_pairs_and_balanced():
    assert Options().class_weights is None
    assert Options(class_weights="1,3").class_weights == (1.0, 3.0)
    assert Options(class_weights=" 0.5 , 2e0 ").class_weights == (0.5, 2.0)
    assert Options(class_weights="0,1").class_weights == (0.0, 1.0)
    assert Options(class_weights=(2, 0.25)).class_weights == (2.0, 0.25)
    assert Options(class_weights="balanced").class_weights == "balanced"
    assert parse_class_weights(None) is None


@pytest.mark.parametrize("bad", ["1", "a,b", "-1,2", "0,0", "nan,1", "1,inf", "1,2,3", "", "balance", (1.0,), 3.0])
def test_class_weights_option_rejects(bad):
    with pytest.raises(ValueError):
        Options(class_weights=bad)


def test_balanced_class_weights():
    mask = np.array([[0.0, 0.9], [0.1, 0.49]])          # 1 road pixel in 4 (binarised at 0.5)
    w0, w1 = balanced_class_weights(mask)
    assert w0 == pytest.approx(2.0 / 3.0, rel=1e-15) and w1 == 2.0
    # the mean weight over the data is 1, and each class carries half of the total
    gt = (np.random.RandomState(0).rand(3, 16, 16) < 0.2).astype(np.float64)
    w0, w1 = balanced_class_weights(gt)
    n1 = gt.sum()
    n0 = gt.size - n1
    assert (w0 * n0 + w1 * n1) / gt.size == pytest.approx(1.0, rel=1e-12)
    assert w0 * n0 == pytest.approx(w1 * n1, rel=1e-12)
    assert balanced_class_weights(gt >= 0.5) == (w0, w1)
    for one_class in (np.zeros((4, 4)), np.ones((4, 4))):
        with pytest.raises(ValueError):
            balanced_class_weights(one_class)


def test_command_line_flag():
    assert [d for d in EXTRA_FLAG_DEFS if d[0] == "class_weights"][0][1:3] == (str, None)
    assert parse_options([]).class_weights is None
    assert parse_options(["--class_weights=1,3"]).class_weights == (1.0, 3.0)
    assert parse_options(["--class_weights", "balanced"]).class_weights == "balanced"
    with pytest.raises(ValueError):
        parse_options(["--class_weights=0,0"])
