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


@pytest.mark.parametrize("shape,iters", CASES, ids=["%s-%d" % (TU.shape_id(s), i) for s, i in CASES])
def test_thin_entry(shape, iters, placement="aligned"):
    prob = CU.float_bank(shape)
    labels64 = TU.mixed_labels(shape)
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
    assert counts.min() > 20 and (info.any() == (iters == TU.K + 1)), what
    assert got["skel_pred"].tobytes() == sp.tobytes() and got["pred_only"].tobytes() == sp.tobytes(), what
    assert got["skel_true"].tobytes() == st.tobytes() and got["true_only"].tobytes() == st.tobytes(), what
    assert np.array_equal(got["acc"], counts) and got["info"].view(np.uint32).tobytes() == info.tobytes(), what
    assert got["info_pred"].view(np.uint32).tobytes() == info.tobytes(), what
    free = hostio.mask_thin(prob, TU.THRESHOLD, None, iters)
    assert got["no_labels"].tobytes() == free[0].tobytes() and got["info_free"].view(np.uint32).tobytes() == free[3].tobytes(), what


# ------------------------------------------------------------------------------------------- the registry (tests/test_thin_host.py)
# launching entry of include/rsu_thin.h -> the cases that launch it inside an arena (HELPERS: what a case calls it through)
FENCED = {"rsu_mask_thin": ["test_thin_entry"]}
HELPERS = {"test_thin_entry": (_launch,)}
