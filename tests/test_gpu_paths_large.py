"""-m gpu: rsu_segment_paths at the largest batch rsu_paths.h admits at the largest side -- 127 images of 1024 x 1024, whose arc buffers take
0x7f000000 bytes each.

The kernels number an arc 2 * (n H W + index) + slot in 32 bits and address the two arc buffers, the pixel plane and the rows' arrays
behind them in one workspace of 4.5 GiB: whether every offset stays in range shows only when the last image's arcs end just below 2^31
bytes. Chains are drawn in the first and the last image alone (the last image is the first one turned by 180 degrees, so it ends in the
very last pixel), in rsu_line_segments' formats; those two images are held to hostio.segment_paths run on them alone, byte for byte; every
other image has no segment and must write four zeros of info, zero pos, and nothing else. No whole tensor comes to the host."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import hiputil as hu  # noqa: E402
from tests import large_util as lu  # noqa: E402
from tests import paths_util as PU  # noqa: E402
from road_segmentation_unet_amd import hostio  # noqa: E402
from road_segmentation_unet_amd._lib import call, lib  # noqa: E402

S = PU.MAX_SIDE
N = 127
CAP, MAX_LEN, MAX_POINTS = 16, 512, 4096
LIVE = ((0, 0), (N - 1, 1))


@pytest.fixture(autouse=True)
def _large_test():
    lu.need_memory()
    yield
    lu.done()


def _chains():
    """flat pixel lists of the first image: a line from pixel 0 along the first row, a line down the last column to the last pixel, a
    diagonal through five tiles in both axes, a hollow square (a ring), a solid block (branched), a line of MAX_LEN + 1 pixels (too long)"""
    at = lambda y, x: y * S + x   # noqa: E731
    ring = [at(500, x) for x in range(60, 70)] + [at(509, x) for x in range(60, 70)] + [at(y, 60) for y in range(501, 509)] + \
        [at(y, 69) for y in range(501, 509)]
    return [[at(0, x) for x in range(100)], [at(y, S - 1) for y in range(900, S)], [at(100 + i, 100 + i) for i in range(300)], ring,
            [at(y, x) for y in range(700, 703) for x in range(200, 203)], [at(800, x) for x in range(100, 100 + MAX_LEN + 1)]]


@functools.lru_cache(maxsize=None)
def _live():
    """(seg [2, S, S], edges [2, CAP, 8], counts [2, 4]) of the first and the last image, and hostio.segment_paths of them: computed once"""
    seg = np.zeros((2, S * S), np.int32)
    edges = np.full((2, CAP, 8), PU.FILL, np.int32)
    counts = np.zeros((2, 4), np.int32)
    for k in range(2):
        chains = [np.sort(np.array(c) if k == 0 else S * S - 1 - np.array(c)) for c in _chains()]
        chains.sort(key=lambda c: c[0])      # ascending label
        for r, c in enumerate(chains):
            seg[k, c] = c[0] + 1
            edges[k, r] = (c[0] + 1, c.size, 0, 0, 0, 0, 0, 0)
        counts[k, 0] = len(chains)
    seg = seg.reshape(2, S, S)
    return seg, edges, counts, hostio.segment_paths(seg, edges, counts, 0, MAX_LEN, MAX_POINTS, fill=PU.FILL)


def test_first_and_last_image_at_the_limit():
    assert N * S * S * 16 < lu.LIMIT <= (N + 1) * S * S * 16
    seg, edges, counts, want = _live()
    paths, offsets, kind, pos, info = want
    assert info.tolist() == [[560, 3, 1, 2]] * 2 and sorted(kind[0, :6].tolist()) == [0, 0, 0, 1, 2, 3]
    assert paths[0, 0] == 0 and S * S - 1 in paths[1, :560] and seg[1, -1, -1] != 0
    new = lambda shape, v: torch.full(shape, v, dtype=torch.int32, device=hu.DEV)   # noqa: E731
    st, et, ct = torch.zeros((N, S, S), dtype=torch.int32, device=hu.DEV), new((N, CAP, 8), PU.FILL), torch.zeros((N, 4), dtype=torch.int32, device=hu.DEV)
    for n, k in LIVE:
        st[n].copy_(torch.from_numpy(seg[k]))
        et[n].copy_(torch.from_numpy(edges[k]))
        ct[n].copy_(torch.from_numpy(counts[k]))
    need = int(lib().rsu_paths_ws_bytes(N, S, S, CAP, MAX_LEN))
    assert need == PU.ws_layout(N, S, S, CAP, MAX_LEN) > 1 << 32
    ws = torch.full((need // 8,), 0x7FA57FA57FA57FA5, dtype=torch.int64, device=hu.DEV)
    gp, go, gk, gi = new((N, MAX_POINTS), PU.FILL), new((N, CAP + 1), PU.FILL), new((N, CAP), PU.FILL), new((N, 4), PU.FILL)
    gpos = new((N, S, S), PU.FILL)
    args = [hu.ptr(st), hu.ptr(et), hu.ptr(ct), 0, CAP, MAX_LEN, MAX_POINTS, hu.ptr(gp), hu.ptr(go), hu.ptr(gk), hu.ptr(gpos), hu.ptr(gi), hu.ptr(ws)]
    call("rsu_segment_paths", *args, N, S, S, hu.stream())
    for n, k in LIVE:
        for name, g, w in zip(PU.NAMES, (gp, go, gk, gpos, gi), want):
            assert g[n].cpu().numpy().tobytes() == w[k].tobytes(), (n, name)
    # the images between them: zero info, offsets[n][0] = 0, nothing ordered, nothing else written
    mid = slice(1, N - 1)
    assert not bool(gi[mid].any().item()) and not bool(go[mid, 0].any().item()) and bool((go[mid, 1:] == PU.FILL).all().item())
    assert bool((gp[mid] == PU.FILL).all().item()) and bool((gk[mid] == PU.FILL).all().item())
    for n0 in range(1, N - 1, 32):
        assert not bool(gpos[n0:min(n0 + 32, N - 1)].any().item()), n0
    # one image further is refused, before anything is launched
    assert lib().rsu_segment_paths(*args, N + 1, S, S, hu.stream()) == -7
    lu.done(st, et, ct, ws, gp, go, gk, gi, gpos)
