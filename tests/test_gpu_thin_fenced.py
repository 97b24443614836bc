"""-m gpu: the launching entry point of include/rsu_thin.h inside a fenced arena (tests/fence_util.py), as
tests/test_gpu_distance_fenced.py holds those of include/rsu_distance.h: rsu_mask_thin with both outputs, acc and info; either output
alone; without labels -- at (3, 63, 65): one row tile, three word columns, the third one pixel wide, the last image ignored altogether --
and at (2, 230, 97): three row tiles and four word columns, all partial; converged (64 iterations) and truncated in the second step
launch (K + 1 = 9). The workspace has exactly rsu_thin_ws_bytes bytes and starts as pattern; acc is a state the case zeroes. After Arena.check
the results are compared with hostio.mask_thin byte for byte: a NaN pattern that reached a result would show there.

FENCED is the registry tests/test_thin_host.py checks against include/rsu_thin.h without a GPU."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import components_util as CU  # noqa: E402
from tests import fence_util as F  # noqa: E402
from tests import hiputil as hu  # noqa: E402
from tests import thin_util as TU  # noqa: E402
from road_segmentation_unet_amd import hostio  # noqa: E402
from road_segmentation_unet_amd._lib import call, lib  # noqa: E402

CASES = [((3, 63, 65), 64), ((2, 230, 97), 64), ((2, 230, 97), TU.K + 1)]


def _launch(A, shape, iters, st):
    """both skeletons with the counts and info; either alone; the prediction's without labels"""
    p = lambda n: hu.ptr(A[n])  # noqa: E731
    call("rsu_mask_thin", p("prob"), TU.THRESHOLD, p("labels64"), iters, p("skel_pred"), p("skel_true"), p("acc"), p("info"), p("ws"), *shape, st)
    call("rsu_mask_thin", p("prob"), TU.THRESHOLD, p("labels64"), iters, p("pred_only"), None, None, p("info_pred"), p("ws"), *shape, st)
    call("rsu_mask_thin", p("prob"), TU.THRESHOLD, p("labels64"), iters, None, p("true_only"), None, None, p("ws"), *shape, st)
    call("rsu_mask_thin", p("prob"), TU.THRESHOLD, None, iters, p("no_labels"), None, None, p("info_free"), p("ws"), *shape, st)


def _case(prob, labels64, shape, iters, placement, truncated):
    nbytes = int(lib().rsu_thin_ws_bytes(*shape, iters))
    assert nbytes > 0 and nbytes % 8 == 0
    specs = [F.f32("prob", prob), F.raw("labels64", labels64)]
    specs += [F.out(n, shape, torch.float32) for n in ("skel_pred", "pred_only", "no_labels")]
    specs += [F.out(n, shape, torch.int64) for n in ("skel_true", "true_only")]
    specs += [F.out(n, (shape[0], 2), torch.int32) for n in ("info", "info_pred", "info_free")]
    specs += [F.state("acc", np.zeros(4, np.int64)), F.ws("ws", nbytes // 8, dtype=torch.int64)]
    A = F.Arena(hu.DEV, specs, placement=placement)
    _launch(A, shape, iters, hu.stream())
    what = "thin fenced %s, %d iterations" % (shape, iters)
    A.check(what)
    got = {s.name: A[s.name].cpu().numpy() for s in specs if s.kind in ("out", "state")}
    sp, st, counts, info = hostio.mask_thin(prob, TU.THRESHOLD, labels64, iters)
    assert counts.min() > 20 and (info.any() == truncated), what
    assert got["skel_pred"].tobytes() == sp.tobytes() and got["pred_only"].tobytes() == sp.tobytes(), what
    assert got["skel_true"].tobytes() == st.tobytes() and got["true_only"].tobytes() == st.tobytes(), what
    assert np.array_equal(got["acc"], counts) and got["info"].view(np.uint32).tobytes() == info.tobytes(), what
    assert got["info_pred"].view(np.uint32).tobytes() == info.tobytes(), what
    free = hostio.mask_thin(prob, TU.THRESHOLD, None, iters)
    assert got["no_labels"].tobytes() == free[0].tobytes() and got["info_free"].view(np.uint32).tobytes() == free[3].tobytes(), what


@pytest.mark.parametrize("shape,iters", CASES, ids=["%s-%d" % (TU.shape_id(s), i) for s, i in CASES])
def test_thin_entry(shape, iters, placement="aligned"):
    _case(CU.float_bank(shape), TU.mixed_labels(shape), shape, iters, placement, iters == TU.K + 1)


EARLY_SHAPE, EARLY_ITERS = (2, 230, 97), 64


def early_inputs():
    """(prob, labels64) at EARLY_SHAPE whose images reach their fixed points at different step launches. Image 0: bars three pixels thick
    on both sides, at their fixed point inside the first step launch (launch 0 deletes, launch 1 finds nothing and leaves a count of 0,
    the launches behind it return at once). Image 1: solid blocks 80 and 60 pixels wide, still being thinned when the first launch ends
    and at their fixed point long before iteration 64; a few of its labels are ignored. tests/test_ws_history_host.py proves both on
    the host."""
    pred, true = np.zeros(EARLY_SHAPE, bool), np.zeros(EARLY_SHAPE, bool)
    pred[0, 20:23, 5:90] = pred[0, 120:123, 3:70] = pred[0, 30:200, 40:43] = True
    true[0, 60:63, 8:95] = true[0, 10:220, 70:73] = True
    pred[1, 40:200, 10:90] = True
    true[1, 25:215, 20:80] = True
    labels64 = true.astype(np.int64)
    labels64[1, 100:104, 0:6] = -1
    labels64[1, 0:3, 90:97] = 2
    return CU.prob_of(pred), labels64


def test_thin_converges_per_image(placement="aligned"):
    """one image at its fixed point inside the first step launch, the other some launches later: the counters differ per image and per
    launch, so a workspace that holds another call's counters holds a 0 where a launch ran and a count where one returned at once"""
    prob, labels64 = early_inputs()
    _case(prob, labels64, EARLY_SHAPE, EARLY_ITERS, placement, False)


# ------------------------------------------------------------------------------------------- the registry (tests/test_thin_host.py)
# launching entry of include/rsu_thin.h -> the cases that launch it inside an arena (HELPERS: what a case calls it through)
FENCED = {"rsu_mask_thin": ["test_thin_entry", "test_thin_converges_per_image"]}
HELPERS = {"test_thin_entry": (_case, _launch), "test_thin_converges_per_image": (_case, _launch)}
