"""-m gpu: the launching entry point of include/rsu_segments.h inside a fenced arena (tests/fence_util.py), as
tests/test_gpu_graph_fenced.py holds that of include/rsu_graph.h: rsu_line_segments with every output and acc; with the tables and counts
alone; without labels -- at (3, 63, 65): two labelling tiles, seventeen compaction blocks, the last one partial, the last image ignored
altogether -- and at (2, 230, 97): eight labelling tiles and two merge levels; on the float bank (thick masks, mostly zone) and on a thinned
pair. The workspace has exactly rsu_segments_ws_bytes bytes and starts as pattern; acc is a state the case zeroes; the tables start as
pattern, so rows past the count (or past the capacity, which the larger float case exceeds) must hold it still. After Arena.check the
results are compared with hostio.line_segments byte for byte.

FENCED is the registry tests/test_segments_host.py checks against include/rsu_segments.h without a GPU."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import components_util as CU  # noqa: E402
from tests import fence_util as F  # noqa: E402
from tests import hiputil as hu  # noqa: E402
from tests import segments_util as SU  # noqa: E402
from tests import thin_util as TU  # noqa: E402
from road_segmentation_unet_amd import hostio  # noqa: E402
from road_segmentation_unet_amd._lib import call, lib  # noqa: E402

CASES = [(s, k) for s in ((3, 63, 65), (2, 230, 97)) for k in ("floats", "thinned")]
CAP = 512
MAPS = ("seg_pred", "seg_true", "node_pred", "node_true", "seg_free", "node_free")
TABLES = ("edges_pred", "edges_true", "edges_pred2", "edges_true2", "edges_free")


def _launch(A, shape, st):
    """every output with acc; the tables and counts alone; the prediction's outputs without labels"""
    p = lambda n: hu.ptr(A[n])  # noqa: E731
    T = SU.THRESHOLD
    call("rsu_line_segments", p("prob"), T, p("labels64"), CAP, p("edges_pred"), p("edges_true"), p("counts"), p("seg_pred"), p("seg_true"),
         p("node_pred"), p("node_true"), p("acc"), p("ws"), *shape, st)
    call("rsu_line_segments", p("prob"), T, p("labels64"), CAP, p("edges_pred2"), p("edges_true2"), p("counts2"), None, None, None, None, None,
         p("ws"), *shape, st)
    call("rsu_line_segments", p("prob"), T, None, CAP, p("edges_free"), None, p("counts_free"), p("seg_free"), None, p("node_free"), None,
         p("acc_free"), p("ws"), *shape, st)


@pytest.mark.parametrize("shape,kind", CASES, ids=["%s-%s" % (SU.shape_id(s), k) for s, k in CASES])
def test_segments_entry(shape, kind, placement="aligned"):
    if kind == "floats":
        prob, labels64 = CU.float_bank(shape), TU.mixed_labels(shape)
    else:
        prob, labels64 = (np.array(a) for a in SU.pair("smooth1.5~smooth3", shape, 0))
    nbytes = int(lib().rsu_segments_ws_bytes(*shape, CAP))
    assert nbytes > 0 and nbytes % 8 == 0
    specs = [F.f32("prob", prob), F.raw("labels64", labels64)]
    specs += [F.out(n, (shape[0], CAP, 8), torch.int32) for n in TABLES]
    specs += [F.out(n, shape, torch.int32) for n in MAPS]
    specs += [F.out(n, (shape[0], 4), torch.int32) for n in ("counts", "counts2", "counts_free")]
    specs += [F.state("acc", np.zeros((2, 8), np.int64)), F.state("acc_free", np.zeros((2, 8), np.int64)), F.ws("ws", nbytes // 8, dtype=torch.int64)]
    A = F.Arena(hu.DEV, specs, placement=placement)
    fill = {n: A[n].cpu().numpy().copy() for n in TABLES}
    _launch(A, shape, hu.stream())
    what = "segments fenced %s, %s" % (shape, kind)
    A.check(what)
    got = {s.name: A[s.name].cpu().numpy() for s in specs if s.kind in ("out", "state")}
    ep, et, counts, sp, st, npd, nt, acc = hostio.line_segments(prob, SU.THRESHOLD, labels64, CAP)
    assert counts[:, 0].max() > 0 and counts[:, 2].max() > 0, what
    assert kind != "floats" or shape[1] < 200 or counts[0, 0] > CAP      # (the thick noisy mask of the larger case overflows the table)
    assert counts[:, 1].max() > 0 and counts[:, 3].max() > 0, what

    def rows(name, want, k):   # the stored rows; behind them the pattern the arena put there
        for n in range(shape[0]):
            c = min(int(k[n]), CAP)
            assert got[name][n, :c].tobytes() == want[n, :c].tobytes(), (what, name, n)
            assert got[name][n, c:].tobytes() == fill[name][n, c:].tobytes(), (what, name, n, "rows past the count were written")
    rows("edges_pred", ep, counts[:, 0])
    rows("edges_pred2", ep, counts[:, 0])
    rows("edges_true", et, counts[:, 2])
    rows("edges_true2", et, counts[:, 2])
    assert got["counts"].tobytes() == counts.tobytes() and got["counts2"].tobytes() == counts.tobytes(), what
    for name, want in (("seg_pred", sp), ("seg_true", st), ("node_pred", npd), ("node_true", nt)):
        assert got[name].tobytes() == want.tobytes(), (what, name)
    assert np.array_equal(got["acc"], acc), what
    free = hostio.line_segments(prob, SU.THRESHOLD, None, CAP)
    assert not free[2][:, 2:].any() and not free[7][1].any()
    rows("edges_free", free[0], free[2][:, 0])
    assert got["counts_free"].tobytes() == free[2].tobytes() and got["seg_free"].tobytes() == free[3].tobytes(), what
    assert got["node_free"].tobytes() == free[5].tobytes() and np.array_equal(got["acc_free"], free[7]), what


# ------------------------------------------------------------------------------------------- the registry (tests/test_segments_host.py)
# launching entry of include/rsu_segments.h -> the cases that launch it inside an arena (HELPERS: what a case calls it through)
FENCED = {"rsu_line_segments": ["test_segments_entry"]}
HELPERS = {"test_segments_entry": (_launch,)}
