"""-m gpu: the two launching entry points of include/rsu_routes.h inside a fenced arena (tests/fence_util.py), as
tests/test_gpu_paths_fenced.py holds that of include/rsu_paths.h, and under the placements and workspace fills that
tests/test_gpu_aligned_min.py and tests/test_gpu_ws_history.py run for the entries of the first ten headers (their registries enumerate
exactly those ten, so this header's runs live here): rsu_graph_routes on both sides of a thinned pair (unpruned: 404, 395, 139 and 115
nodes in tables of 256 rows, so nodes are dropped on one side and rows of every table stay untouched; pruned: 196 .. 215 and 77 .. 79
nodes), then rsu_route_score in both directions. The workspace has exactly rsu_routes_ws_bytes bytes. After Arena.check the results are
compared with hostio.graph_routes and hostio.route_score byte for byte; elements the entries do not touch must still hold the arena's
pattern.

  test_routes_entries                 every payload on a 256-byte boundary, the workspace as pattern;
  test_routes_entries_at_their_minimum  every payload at a 256-byte boundary plus exactly its alignment (int32: 4, acc: 8);
  test_routes_workspace_history       the workspace zeroed, 0xFF-filled and rolled, put back in front of every call: the bytes of the pattern run.

FENCED is the registry tests/test_routes_host.py checks without a GPU."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import fence_util as F  # noqa: E402
from tests import hiputil as hu  # noqa: E402
from tests import routes_util as RU  # noqa: E402
from road_segmentation_unet_amd import hostio  # noqa: E402
from road_segmentation_unet_amd._lib import call, lib  # noqa: E402

PATTERN32 = 0x7FA57FA5      # what an int32 of an arena holds before a launch
NAME, SHAPE, MAX_NODES = "smooth1.5~smooth3", (2, 230, 97), 256
CASES = {"unpruned": 0, "pruned": 8}      # case -> min_branch
OUTS = tuple("%s%d" % (n, s) for s in (0, 1) for n in ("nodes", "dist", "info", "match"))
ACCS = ("acc0", "acc1")
ALIGN = dict({n: 4 for n in ("map0", "map1", "edges0", "edges1", "counts", "ws") + OUTS}, acc0=8, acc1=8)      # the header's align notes


def _launch(A, st):
    """both sides' graphs, the workspace from the placement's fill both times; then the score from side 0 to side 1 and back"""
    q = lambda n: hu.ptr(A[n])  # noqa: E731
    cap = int(A["edges0"].shape[1])
    for side in (0, 1):
        A.refill("ws")
        call("rsu_graph_routes", q("map%d" % side), q("edges%d" % side), q("counts"), side, cap, MAX_NODES, q("nodes%d" % side),
             q("dist%d" % side), q("info%d" % side), q("ws"), *SHAPE, st)
    for a in (0, 1):
        b = 1 - a
        call("rsu_route_score", q("nodes%d" % a), q("dist%d" % a), q("info%d" % a), q("nodes%d" % b), q("dist%d" % b), q("info%d" % b), MAX_NODES,
             RU.SLACK, q("match%d" % a), q("acc%d" % a), SHAPE[0], st)


def _case(case, placement="aligned"):
    """one fenced run; returns {output name: bytes}"""
    L = CASES[case]
    inputs = [tuple(np.array(a) for a in RU.bank_inputs(NAME, SHAPE, L, side)) for side in (0, 1)]
    N = SHAPE[0]
    nbytes = int(lib().rsu_routes_ws_bytes(*SHAPE, MAX_NODES))
    assert nbytes == RU.ws_layout(*SHAPE, MAX_NODES) and nbytes % 4 == 0
    specs = [F.raw("counts", inputs[0][2])]
    for side in (0, 1):
        specs += [F.raw("map%d" % side, inputs[side][0]), F.raw("edges%d" % side, inputs[side][1]),
                  F.out("nodes%d" % side, (N, MAX_NODES, 4), torch.int32), F.out("dist%d" % side, (N, MAX_NODES, MAX_NODES), torch.int32),
                  F.out("info%d" % side, (N, 4), torch.int32), F.out("match%d" % side, (N, MAX_NODES), torch.int32),
                  F.state("acc%d" % side, np.zeros(4, np.int64))]
    specs.append(F.ws("ws", nbytes // 4, dtype=torch.int32))
    A = F.Arena(hu.DEV, specs, placement=placement)
    if A.placement.mode == "minimum":      # a multiple of its number and of nothing larger
        for s in specs:
            assert A[s.name].data_ptr() % (2 * ALIGN[s.name]) == ALIGN[s.name], s.name
    _launch(A, hu.stream())
    what = "routes fenced %s" % case
    A.check(what)
    got = {n: A[n].cpu().numpy() for n in OUTS + ACCS}
    g = [hostio.graph_routes(*inputs[side], side, MAX_NODES, fill=PATTERN32) for side in (0, 1)]
    for side in (0, 1):
        for name, w in zip(RU.NAMES, g[side]):
            assert got["%s%d" % (name, side)].tobytes() == w.tobytes(), (what, name, side)
        match, acc = hostio.route_score(*g[side], *g[1 - side], RU.SLACK, fill=PATTERN32)
        assert got["match%d" % side].tobytes() == match.tobytes() and got["acc%d" % side].tolist() == acc.tolist(), (what, "score", side)
        assert acc[0] > 500, what      # work
    assert (g[1][1] == PATTERN32).any() and (g[1][0] == PATTERN32).any() and (got["match1"] == PATTERN32).any(), what      # untouched elements
    assert (g[0][2][:, 0] > MAX_NODES).all() == (L == 0)
    return {n: v.tobytes() for n, v in got.items()}


@pytest.mark.parametrize("case", sorted(CASES))
def test_routes_entries(case):
    _case(case)


@pytest.mark.parametrize("case", sorted(CASES))
def test_routes_entries_at_their_minimum(case):
    assert _case(case, F.Placement("minimum", [{"acc0": 8, "acc1": 8}])) == _case(case)


@pytest.mark.parametrize("fill", ("zeros", "ones", "rolled"))
@pytest.mark.parametrize("case", sorted(CASES))
def test_routes_workspace_history(case, fill):
    first = F.Placement("aligned", fill="pattern")
    want = _case(case, first)
    snaps = first.workspaces()
    assert list(snaps) == [(0, "ws")]
    got = _case(case, F.Placement("aligned", fill=fill, snapshots=snaps))
    bad = [n for n in OUTS + ACCS if got[n] != want[n]]
    assert not bad, "workspace fill %r changed %s" % (fill, bad)


# ------------------------------------------------------------------------------------------- the registry (tests/test_routes_host.py)
_TESTS = ["test_routes_entries", "test_routes_entries_at_their_minimum", "test_routes_workspace_history"]
FENCED = {"rsu_graph_routes": _TESTS, "rsu_route_score": _TESTS}
HELPERS = {n: (_case, _launch) for n in _TESTS}
