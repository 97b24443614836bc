"""-m gpu: the launching entry point of include/rsu_graph.h inside a fenced arena (tests/fence_util.py), as tests/test_gpu_thin_fenced.py
holds that of include/rsu_thin.h: rsu_skeleton_graph with all four outputs and acc; each output alone; without labels -- at (3, 63, 65):
one row tile, three word columns, the third one pixel wide, the last image ignored altogether -- and at (2, 230, 97): three row tiles and
four word columns, all partial; at min_branch 0 (no prune step, the one-plane workspace), R + 1 (the second delete and regrow launches
run) and 64 (eleven launches). The workspace has exactly rsu_graph_ws_bytes bytes and starts as pattern; acc is a state the case zeroes.
After Arena.check the results are compared with hostio.skeleton_graph byte for byte: a NaN pattern that reached a result would show there.

FENCED is the registry tests/test_graph_host.py checks against include/rsu_graph.h without a GPU."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import components_util as CU  # noqa: E402
from tests import fence_util as F  # noqa: E402
from tests import graph_util as GU  # noqa: E402
from tests import hiputil as hu  # noqa: E402
from tests import thin_util as TU  # noqa: E402
from road_segmentation_unet_amd import hostio  # noqa: E402
from road_segmentation_unet_amd._lib import call, lib  # noqa: E402

CASES = [(s, b) for s in ((3, 63, 65), (2, 230, 97)) for b in (0, GU.R + 1, GU.MAX_BRANCH)]


def _launch(A, shape, b, st):
    """all four outputs with the counts; each alone; the prediction's two without labels"""
    p = lambda n: hu.ptr(A[n])  # noqa: E731
    T = GU.THRESHOLD
    call("rsu_skeleton_graph", p("prob"), T, p("labels64"), b, p("out_pred"), p("out_true"), p("junc_pred"), p("junc_true"), p("acc"), p("ws"),
         *shape, st)
    call("rsu_skeleton_graph", p("prob"), T, p("labels64"), b, p("pred_only"), None, None, None, None, p("ws"), *shape, st)
    call("rsu_skeleton_graph", p("prob"), T, p("labels64"), b, None, p("true_only"), None, None, None, p("ws"), *shape, st)
    call("rsu_skeleton_graph", p("prob"), T, p("labels64"), b, None, None, p("jpred_only"), None, None, p("ws"), *shape, st)
    call("rsu_skeleton_graph", p("prob"), T, p("labels64"), b, None, None, None, p("jtrue_only"), None, p("ws"), *shape, st)
    call("rsu_skeleton_graph", p("prob"), T, None, b, p("no_labels"), None, p("jno_labels"), None, p("acc_free"), p("ws"), *shape, st)


def _case(prob, labels64, shape, b, placement):
    nbytes = int(lib().rsu_graph_ws_bytes(*shape, b))
    assert nbytes > 0 and nbytes % 8 == 0
    specs = [F.f32("prob", prob), F.raw("labels64", labels64)]
    specs += [F.out(n, shape, torch.float32) for n in ("out_pred", "junc_pred", "pred_only", "jpred_only", "no_labels", "jno_labels")]
    specs += [F.out(n, shape, torch.int64) for n in ("out_true", "junc_true", "true_only", "jtrue_only")]
    specs += [F.state("acc", np.zeros(8, np.int64)), F.state("acc_free", np.zeros(8, np.int64)), F.ws("ws", nbytes // 8, dtype=torch.int64)]
    A = F.Arena(hu.DEV, specs, placement=placement)
    _launch(A, shape, b, hu.stream())
    what = "graph fenced %s, min_branch %d" % (shape, b)
    A.check(what)
    got = {s.name: A[s.name].cpu().numpy() for s in specs if s.kind in ("out", "state")}
    op, ot, jp, jt, counts = hostio.skeleton_graph(prob, GU.THRESHOLD, labels64, b)
    assert (counts[[0, 3, 4, 7]] > 0).all(), what      # (noise pruned deep enough has loops and junctions left, but no end)
    assert got["out_pred"].tobytes() == op.tobytes() and got["pred_only"].tobytes() == op.tobytes(), what
    assert got["out_true"].tobytes() == ot.tobytes() and got["true_only"].tobytes() == ot.tobytes(), what
    assert got["junc_pred"].tobytes() == jp.tobytes() and got["jpred_only"].tobytes() == jp.tobytes(), what
    assert got["junc_true"].tobytes() == jt.tobytes() and got["jtrue_only"].tobytes() == jt.tobytes(), what
    assert np.array_equal(got["acc"], counts), what
    free = hostio.skeleton_graph(prob, GU.THRESHOLD, None, b)
    assert got["no_labels"].tobytes() == free[0].tobytes() and got["jno_labels"].tobytes() == free[2].tobytes(), what
    assert np.array_equal(got["acc_free"], free[4]) and not free[4][4:].any(), what


@pytest.mark.parametrize("shape,b", CASES, ids=["%s-%d" % (GU.shape_id(s), b) for s, b in CASES])
def test_graph_entry(shape, b, placement="aligned"):
    _case(CU.float_bank(shape), TU.mixed_labels(shape), shape, b, placement)


EARLY_SHAPE = (2, 230, 97)


def _theta(m, y0, y1, x0, x1):
    """a one-pixel rectangle outline with a bar across it: four junctions, no end"""
    m[y0, x0:x1 + 1] = m[y1, x0:x1 + 1] = m[(y0 + y1) // 2, x0:x1 + 1] = True
    m[y0:y1 + 1, x0] = m[y0:y1 + 1, x1] = True


def early_inputs():
    """(prob, labels64) at EARLY_SHAPE, for min_branch = MAX_BRANCH (four delete and five regrow launches), whose images and sides end
    their delete phase at different launches. Image 0, prediction: an outline with a bar across it and a spur of five pixels -- the first
    delete launch removes the spur, the second finds nothing and leaves a count of 0, the other launches of both phases return at once.
    Image 0, truth: the same without a spur and a lone line of nine pixels, gone in the first five rounds; the second launch counts 0.
    Image 1, prediction: a line of 200 pixels, shortened by every round of every delete launch and regrown to its full length. Image 1,
    truth: an outline with a spur of 40 pixels, deleted by the first three launches; the fourth counts 0 and nothing is regrown. A few
    labels of image 1 are ignored. tests/test_ws_history_host.py proves this on the host."""
    pred, true = np.zeros(EARLY_SHAPE, bool), np.zeros(EARLY_SHAPE, bool)
    _theta(pred[0], 20, 80, 10, 70)
    pred[0, 81:86, 40] = True
    _theta(true[0], 100, 180, 20, 90)
    true[0, 200, 30:39] = True
    pred[1, 15:215, 50] = True
    _theta(true[1], 60, 120, 10, 50)
    true[1, 90, 51:91] = True
    labels64 = true.astype(np.int64)
    labels64[1, 200:204, 0:6] = -1
    labels64[1, 0:3, 90:97] = 2
    return CU.prob_of(pred), labels64


def test_graph_converges_per_image(placement="aligned"):
    """every image side ends its delete phase at another launch, one regrows and three do not: the counters differ per image, side and
    launch, so a workspace that holds another call's counters holds a 0 where a launch ran and a count where one returned at once"""
    prob, labels64 = early_inputs()
    _case(prob, labels64, EARLY_SHAPE, GU.MAX_BRANCH, placement)


# ------------------------------------------------------------------------------------------- the registry (tests/test_graph_host.py)
# launching entry of include/rsu_graph.h -> the cases that launch it inside an arena (HELPERS: what a case calls it through)
FENCED = {"rsu_skeleton_graph": ["test_graph_entry", "test_graph_converges_per_image"]}
HELPERS = {"test_graph_entry": (_case, _launch), "test_graph_converges_per_image": (_case, _launch)}
