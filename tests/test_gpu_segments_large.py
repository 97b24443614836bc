"""-m gpu: rsu_line_segments with labels64 at the largest batch rsu_segments.h admits at the largest side -- 127 images of 1024 x 1024, whose
four int32 planes in the workspace take 0x7f000000 bytes.

The kernels form every pixel's offset as plane * H * W + index with up to 4 N planes: whether they stay in range shows only when the last
plane ends just below 2^31 bytes (and far past 2^31 elements' worth of bytes in the workspace as a whole). Only the first and the last
image carry content -- pruned centre-lines of the bank, prepared on the host at 256 x 256 and set into the corners of the images, so
that the host is spared four 1024 x 1024 references' thinning -- and only those are held to hostio.line_segments, byte for byte; every
other image is ignored altogether (labels -1 under a probability above the threshold) and must produce zero counts, no row and nothing
in the maps. No whole tensor comes to the host."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import hiputil as hu  # noqa: E402
from tests import large_util as lu  # noqa: E402
from tests import segments_util as SU  # noqa: E402
from road_segmentation_unet_amd import hostio  # noqa: E402
from road_segmentation_unet_amd._lib import call, lib  # noqa: E402

S = SU.MAX_SIDE
N = 127
CAP = 4096
LIVE = ((0, 0), (N - 1, 1))
Q = 256


@pytest.fixture(autouse=True)
def _large_test():
    lu.need_memory()
    yield
    lu.done()


@functools.lru_cache(maxsize=None)
def _live():
    """(prob float32, labels int64) [2, S, S] of the first and the last image and hostio.line_segments of them: computed once. The
    centre-lines sit in the first image's first rows and columns and in the last image's last ones"""
    p0, l0 = SU.pair("smooth1.5~smooth3", (2, Q, Q), 0)
    p8, l8 = SU.pair("smooth3~smooth1.5", (2, Q, Q), 8)
    prob = np.full((2, S, S), 0.25, np.float32)
    labels = np.zeros((2, S, S), np.int64)
    prob[0, :Q, :Q], labels[0, :Q, :Q] = p0[0], l0[0]
    prob[0, :Q, S - Q:], labels[0, S - Q:, :Q] = p8[0], l8[0]
    prob[1, S - Q:, S - Q:], labels[1, S - Q:, S - Q:] = p0[1], l0[1]
    prob[1, S - Q:, :Q], labels[1, :Q, S - Q:] = p8[1], l8[1]
    labels[:, ::11, ::13] = -1
    prob[:, 3::7, ::5] = np.float32(np.nan)          # outside
    return prob, labels, hostio.line_segments(prob, SU.THRESHOLD, labels, CAP, fill=SU.FILL)


def test_first_and_last_image_at_the_limit():
    assert N * S * S * 16 < lu.LIMIT <= (N + 1) * S * S * 16
    prob, labels, want = _live()
    ep, et, counts, sp, st, npd, nt, acc = want
    assert counts.min() > 50 and counts[:, [0, 2]].max() <= CAP and (acc[:, :4] > 0).all()
    pt = torch.full((N, S, S), 0.75, dtype=torch.float32, device=hu.DEV)
    lt = torch.full((N, S, S), -1, dtype=torch.int64, device=hu.DEV)
    for n, k in LIVE:
        pt[n].copy_(torch.from_numpy(prob[k]))
        lt[n].copy_(torch.from_numpy(labels[k]))
    need = int(lib().rsu_segments_ws_bytes(N, S, S, CAP))
    assert need == SU.ws_layout(N, S, S) > 1 << 32
    ws = torch.full((need // 8,), 0x7FA57FA57FA57FA5, dtype=torch.int64, device=hu.DEV)
    new = lambda shape: torch.full(shape, SU.FILL, dtype=torch.int32, device=hu.DEV)   # noqa: E731
    gep, get, gc = new((N, CAP, 8)), new((N, CAP, 8)), new((N, 4))
    maps = [new((N, S, S)) for _ in range(4)]
    gacc = torch.zeros((2, 8), dtype=torch.int64, device=hu.DEV)
    call("rsu_line_segments", hu.ptr(pt), SU.THRESHOLD, hu.ptr(lt), CAP, hu.ptr(gep), hu.ptr(get), hu.ptr(gc), hu.ptr(maps[0]), hu.ptr(maps[1]),
         hu.ptr(maps[2]), hu.ptr(maps[3]), hu.ptr(gacc), hu.ptr(ws), N, S, S, hu.stream())
    for n, k in LIVE:
        assert gc[n].cpu().numpy().tobytes() == counts[k].tobytes(), n
        assert gep[n].cpu().numpy().tobytes() == ep[k].tobytes() and get[n].cpu().numpy().tobytes() == et[k].tobytes(), n
        for g, w in zip(maps, (sp, st, npd, nt)):
            assert g[n].cpu().numpy().tobytes() == w[k].tobytes(), n
    # the images between them: zero counts, no row, nothing in the maps
    assert not bool(gc[1:N - 1].any().item())
    assert bool((gep[1:N - 1] == SU.FILL).all().item()) and bool((get[1:N - 1] == SU.FILL).all().item())
    for g in maps:
        for n0 in range(1, N - 1, 32):
            assert not bool(g[n0:min(n0 + 32, N - 1)].any().item()), n0
    assert np.array_equal(gacc.cpu().numpy(), acc)
    # one image further is refused, before anything is launched
    assert lib().rsu_line_segments(hu.ptr(pt), SU.THRESHOLD, hu.ptr(lt), CAP, hu.ptr(gep), hu.ptr(get), hu.ptr(gc), None, None, None, None, None,
                                   hu.ptr(ws), N + 1, S, S, hu.stream()) == -7
    lu.done(pt, lt, ws, gep, get, gc, gacc, *maps)
