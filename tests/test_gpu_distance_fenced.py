"""-m gpu: the launching entry points of include/rsu_distance.h inside a fenced arena (tests/fence_util.py), as
tests/test_gpu_components_fenced.py holds those of include/rsu_components.h: rsu_mask_distance (both outputs; either alone; without
labels) and rsu_distance_hist at (3, 63, 65) -- one chunk of rows a row short, two strips of columns, the second one column wide -- and at
(2, 130, 67): three chunks and two strips, both partial. The workspace has exactly rsu_distance_ws_bytes bytes and starts as pattern; acc
is a state the case zeroes. After Arena.check the results are compared with the host restatements of hostio.

FENCED is the registry tests/test_distance_host.py checks against include/rsu_distance.h without a GPU."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import components_util as CU  # noqa: E402
from tests import distance_util as DU  # noqa: E402
from tests import fence_util as F  # noqa: E402
from tests import hiputil as hu  # noqa: E402
from road_segmentation_unet_amd import hostio  # noqa: E402
from road_segmentation_unet_amd._lib import call, lib  # noqa: E402

SHAPES = [(3, 63, 65), (2, 130, 67)]


def _launch(A, shape, st):
    """both distances; either alone; the prediction's without labels; the histogram"""
    p = lambda n: hu.ptr(A[n])  # noqa: E731
    call("rsu_mask_distance", p("prob"), DU.THRESHOLD, p("labels64"), p("d2_pred"), p("d2_true"), p("ws"), *shape, st)
    call("rsu_mask_distance", p("prob"), DU.THRESHOLD, p("labels64"), p("pred_only"), None, p("ws"), *shape, st)
    call("rsu_mask_distance", p("prob"), DU.THRESHOLD, p("labels64"), None, p("true_only"), p("ws"), *shape, st)
    call("rsu_mask_distance", p("prob"), DU.THRESHOLD, None, p("no_labels"), None, p("ws"), *shape, st)
    call("rsu_distance_hist", p("prob"), DU.THRESHOLD, p("labels64"), p("acc"), p("ws"), *shape, st)


@pytest.mark.parametrize("shape", SHAPES, ids=[DU.shape_id(s) for s in SHAPES])
def test_distance_entries(shape, placement="aligned"):
    prob = CU.float_bank(shape)
    labels64 = DU.mixed_labels(shape)
    nbytes = int(lib().rsu_distance_ws_bytes(*shape))
    assert nbytes == 4 * int(np.prod(shape))
    specs = [F.f32("prob", prob), F.raw("labels64", labels64)]
    specs += [F.out(n, shape, torch.int32) for n in ("d2_pred", "d2_true", "pred_only", "true_only", "no_labels")]
    specs += [F.state("acc", np.zeros((2, DU.BINS), np.int64)), F.ws("ws", nbytes // 4, dtype=torch.int32)]
    A = F.Arena(hu.DEV, specs, placement=placement)
    _launch(A, shape, hu.stream())
    what = "distance fenced %s" % (shape,)
    A.check(what)
    got = {n: A[n].cpu().numpy() for n in ("d2_pred", "d2_true", "pred_only", "true_only", "no_labels", "acc")}
    d2p, d2t = hostio.mask_distance(prob, DU.THRESHOLD, labels64)
    assert np.array_equal(got["d2_pred"], d2p) and np.array_equal(got["d2_true"], d2t), what
    assert np.array_equal(got["pred_only"], d2p) and np.array_equal(got["true_only"], d2t), what
    assert np.array_equal(got["no_labels"], hostio.mask_distance(prob, DU.THRESHOLD)[0]), what
    want = hostio.distance_hist(prob, DU.THRESHOLD, labels64)
    assert want[0].sum() > 100 and want[1].sum() > 100 and np.array_equal(got["acc"], want), what


# ------------------------------------------------------------------------------------------- the registry (tests/test_distance_host.py)
# launching entry of include/rsu_distance.h -> the cases that launch it inside an arena (HELPERS: what a case calls it through)
FENCED = {
    "rsu_mask_distance": ["test_distance_entries"],
    "rsu_distance_hist": ["test_distance_entries"],
}
HELPERS = {"test_distance_entries": (_launch,)}
