"""-m gpu: rsu_graph_routes at the largest batches rsu_routes.h admits -- 511 images of 1024 x 1024 with 64 nodes' room, whose node_map
takes 0x7fc00000 bytes, and 511 images of 32 x 32 with 1024 nodes' room, whose dist takes as much; 512 is refused in both.

Whether every offset into node_map and into dist stays in range shows only when the last image ends just below 2^31 bytes. Only the first
and the last image are populated (line ends and hand-written rows, in rsu_line_segments' formats; the last image holds a node at its very
last pixel, and in the second case 1024 nodes, so its last distance is the tensor's last element); those two images are held to
hostio.graph_routes run on them alone, byte for byte, and in the second case to hostio.route_score as well; every other image has no node,
returns at once, and must write four zeros of info and nothing else. No whole tensor comes to the host."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import hiputil as hu  # noqa: E402
from tests import large_util as lu  # noqa: E402
from tests import routes_util as RU  # noqa: E402
from road_segmentation_unet_amd import hostio  # noqa: E402
from road_segmentation_unet_amd._lib import call, lib  # noqa: E402

N = 511
# case -> (side of the image, max_nodes, max_edges, nodes of the first and of the last image)
CASES = {"node_map": (1024, 64, 128, (40, 64)), "dist": (32, 1024, 1300, (130, 1024))}


@pytest.fixture(autouse=True)
def _large_test():
    lu.need_memory()
    yield
    lu.done()


@functools.lru_cache(maxsize=None)
def _live(case):
    """(node_map [2, S, S], edges [2, cap, 8], counts [2, 4]) of the first and the last image and hostio.graph_routes of them: computed once"""
    S, max_nodes, cap, nodes = CASES[case]
    m = np.zeros((2, S * S), np.int32)
    e = np.full((2, cap, 8), RU.FILL, np.int32)
    c = np.zeros((2, 4), np.int32)
    for k, count in enumerate(nodes):
        rng = np.random.RandomState(7 + k)
        px = np.sort(rng.choice(S * S - 2, count - 2, replace=False) + 1) if count < S * S else np.arange(1, S * S - 1)
        px = np.concatenate([[0], px, [S * S - 1]])      # the first and the very last pixel of the image are nodes
        m[k, px] = -(px + 1).astype(np.int32)
        rows = RU.chain_rows(count, seed=k) + RU.sparse_rows(count // 8 + 1, seed=k)
        assert len(rows) <= cap
        for r, (a, b, ortho, diag) in enumerate(rows):
            ia, ib = -(int(px[a]) + 1), -(int(px[b]) + 1)
            e[k, r] = (r + 1, ortho + diag + 1, ortho, diag, min(ia, ib), max(ia, ib), 0, 2)
        c[k, 0] = len(rows)
    m = m.reshape(2, S, S)
    return m, e, c, hostio.graph_routes(m, e, c, 0, max_nodes, fill=RU.FILL)


@pytest.mark.parametrize("case", sorted(CASES))
def test_first_and_last_image_at_the_limit(case):
    S, max_nodes, cap, nodes = CASES[case]
    big = S * S if case == "node_map" else max_nodes * max_nodes
    assert N * big * 4 < lu.LIMIT <= (N + 1) * big * 4
    m, e, c, want = _live(case)
    assert want[2][:, :2].tolist() == [[n, n] for n in nodes] and (want[1][1, :nodes[1], :nodes[1]] < RU.INF).all() and m[1, -1, -1] == -S * S
    new = lambda shape, v: torch.full(shape, v, dtype=torch.int32, device=hu.DEV)   # noqa: E731
    mt, et, ct = new((N, S, S), 0), new((N, cap, 8), RU.FILL), new((N, 4), 0)
    for n, k in ((0, 0), (N - 1, 1)):
        mt[n].copy_(torch.from_numpy(m[k]))
        et[n].copy_(torch.from_numpy(e[k]))
        ct[n].copy_(torch.from_numpy(c[k]))
    need = int(lib().rsu_routes_ws_bytes(N, S, S, max_nodes))
    assert need == RU.ws_layout(N, S, S, max_nodes) > 0
    ws = torch.full((need // 4,), 0x7FA57FA5, dtype=torch.int32, device=hu.DEV)
    gn, gd, gi = new((N, max_nodes, 4), RU.FILL), new((N, max_nodes, max_nodes), RU.FILL), new((N, 4), RU.SENTINEL)
    args = [hu.ptr(mt), hu.ptr(et), hu.ptr(ct), 0, cap, max_nodes, hu.ptr(gn), hu.ptr(gd), hu.ptr(gi), hu.ptr(ws)]
    call("rsu_graph_routes", *args, N, S, S, hu.stream())
    for n, k in ((0, 0), (N - 1, 1)):
        for name, g, w in zip(RU.NAMES, (gn, gd, gi), want):
            assert g[n].cpu().numpy().tobytes() == w[k].tobytes(), (n, name)
    # the images between them: zero info and nothing else written
    mid = slice(1, N - 1)
    assert not bool(gi[mid].any().item()) and bool((gn[mid] == RU.FILL).all().item())
    for n0 in range(1, N - 1, 64):
        assert bool((gd[n0:min(n0 + 64, N - 1)] == RU.FILL).all().item()), n0
    if case == "dist":      # the score reads the same tensors: the graph against itself, held to the restatement on the two live images
        match, acc = new((N, max_nodes), RU.FILL), torch.zeros(4, dtype=torch.int64, device=hu.DEV)
        sargs = [hu.ptr(gn), hu.ptr(gd), hu.ptr(gi)] * 2 + [max_nodes, RU.SLACK, hu.ptr(match), hu.ptr(acc)]
        call("rsu_route_score", *sargs, N, hu.stream())
        wm, wa = hostio.route_score(*want, *want, RU.SLACK, fill=RU.FILL)
        assert acc.cpu().numpy().tolist() == wa.tolist() and wa[0] > 500000
        assert match[0].cpu().numpy().tobytes() == wm[0].tobytes() and match[N - 1].cpu().numpy().tobytes() == wm[1].tobytes()
        assert bool((match[mid] == RU.FILL).all().item())
        assert lib().rsu_route_score(*sargs, N + 1, hu.stream()) == -7
        del match, acc
    # one image further is refused, before anything is launched
    assert lib().rsu_graph_routes(*args, N + 1, S, S, hu.stream()) == -7
    lu.done(mt, et, ct, ws, gn, gd, gi)
