"""GPU test: evaluate() with all five mask stages on at once (mask_metrics.MaskMetrics: one accumulator, one reset, one read-back)
against five models that each have one stage on, plus what that stage requires. Integers throughout: every key must be equal."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from tests import test_gpu_graph as TG  # noqa: E402


def _equal(a, b):
    return (isinstance(b, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b)) if isinstance(a, np.ndarray) \
        else (type(a) is type(b) and a == b)


@pytest.mark.parametrize("min_branch", [0, 2])
def test_all_stages_at_once_equal_each_stage_alone(min_branch):
    N = 5                                      # chunks of two: the last one is padded
    X, y = TG._patches(N)
    y[1, :3] = -1                              # a few ignored rows
    lines = dict(validate_centerlines=True, centerline_min_branch=min_branch, relaxed_slack=2)
    m = TG._model(validate_components=True, validate_distances=True, validate_junctions=True, validate_segments=True, **lines)
    thr = round(float(np.median(np.concatenate([c[0].reshape(-1) for c in TG._chunks(m, X, y)]))) * 256.0) / 256.0
    out = m.evaluate(X, y, threshold=thr)
    assert [k for k in m._mask_metrics.lay if "." not in k] == ["components", "distances", "centerlines", "graph", "segments"]
    assert out["components_pred"] > 0 and out["dist_hist"][0, 1:].sum() > 0 and out["cl_len_true"] > 0 and out["junctions_true"] > 0
    assert out["segments_true"] > 0 and out["nodes_pred"] > 0
    alone = [dict(validate_components=True), dict(validate_distances=True, relaxed_slack=2), lines, dict(validate_junctions=True, **lines),
             dict(validate_segments=True, **lines)]
    seen = set()
    for kw in alone:
        one = TG._model(**kw).evaluate(X, y, threshold=thr)
        assert set(one) < set(out), kw
        for k, v in one.items():
            assert _equal(out[k], v), (kw, k, out[k], v)
        seen |= set(one)
    assert seen == set(out)
    # the same model again: the one reset() in front of the pass clears every stage's counters
    again = m.evaluate(X, y, threshold=thr)
    assert list(again) == list(out)
    for k, v in out.items():
        assert _equal(again[k], v), (k, again[k], v)
