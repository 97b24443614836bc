"""-m gpu: rsu_mask_thin with labels64 and skel_true one image short of the 2-GiB limit -- 255 images of 1024 x 1024, 0x7f800000 bytes each,
the largest batch rsu_thin.h admits at the largest side.

The kernels form every pixel's offset as image * H * W + y * W + x and every plane word's as (image * 2 + side) * H * Wq + y * Wq + xw:
whether they stay in range shows only when the last image ends just below 2^31 bytes. Only the first and the last image carry masks of the
bank, and only those are held to hostio.mask_thin, byte for byte; every other image is ignored altogether (labels -1 under a probability
above the threshold), and a reduction on the device asserts that its skel_true is its labels64, its skel_pred empty and its info 0. K + 1
iterations: the second step launch runs, truncated, and the host restatement stays at a few passes over two images. First with skel_pred
NULL, as the issue of this test asks; then with both outputs, which acc requires. No whole tensor comes to the host."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import hiputil as hu  # noqa: E402
from tests import large_util as lu  # noqa: E402
from tests import thin_util as TU  # noqa: E402
from road_segmentation_unet_amd import hostio  # noqa: E402
from road_segmentation_unet_amd._lib import call, lib  # noqa: E402

S = TU.MAX_SIDE
ITERS = TU.K + 1
N = 255


@pytest.fixture(autouse=True)
def _large_test():
    lu.need_memory()
    yield
    lu.done()


@functools.lru_cache(maxsize=None)
def _live():
    """(prob float32, labels int64) [2, S, S] of the first and the last image and hostio.mask_thin of them: computed once"""
    pred = np.stack([TU.masks("smooth6", (1, S, S))[0], TU.masks("rand0.55", (1, S, S))[0]])
    true = np.stack([TU.masks("rand0.45", (1, S, S))[0], TU.masks("smooth3", (1, S, S))[0]])
    labels = true.astype(np.int64)
    labels[:, ::11, ::13] = -1
    prob = np.where(pred, np.float32(0.75), np.float32(0.25)).astype(np.float32)
    prob[:, ::7, ::5] = np.float32(TU.THRESHOLD)     # the threshold itself: inside
    prob[:, 3::7, ::5] = np.float32(np.nan)          # outside
    return prob, labels, hostio.mask_thin(prob, TU.THRESHOLD, labels, ITERS)


def _batch():
    prob, labels, _ = _live()
    pt = torch.full((N, S, S), 0.75, dtype=torch.float32, device=hu.DEV)
    lt = torch.full((N, S, S), -1, dtype=torch.int64, device=hu.DEV)
    for n, k in ((0, 0), (N - 1, 1)):
        pt[n].copy_(torch.from_numpy(prob[k]))
        lt[n].copy_(torch.from_numpy(labels[k]))
    need = int(lib().rsu_thin_ws_bytes(N, S, S, ITERS))
    assert need > 0
    ws = torch.full((need // 8,), 0x7FA57FA57FA57FA5, dtype=torch.int64, device=hu.DEV)
    return pt, lt, ws


def _check_true(st, lt, info):
    _, _, (_, want_t, _, want_i) = _live()
    for n, k in ((0, 0), (N - 1, 1)):
        assert st[n].cpu().numpy().tobytes() == want_t[k].tobytes(), n
        assert info[n].cpu().numpy().view(np.uint32).tobytes() == want_i[k].tobytes(), n
    assert want_i[0, 0] and want_i[1, 1] and not want_i[0, 1]     # (nine iterations finish the noise, not the smooth blobs)
    for n0 in range(1, N - 1, 32):
        n1 = min(n0 + 32, N - 1)
        assert bool((st[n0:n1] == lt[n0:n1]).all().item()), (n0, n1)
    assert not bool(info[1:N - 1].any().item())


def test_skel_true_alone_at_the_limit():
    assert N == lu.n_max(S * S * 8) and N * S * S * 8 < lu.LIMIT <= (N + 1) * S * S * 8
    pt, lt, ws = _batch()
    st = torch.full((N, S, S), -7, dtype=torch.int64, device=hu.DEV)
    info = torch.full((N, 2), -7, dtype=torch.int32, device=hu.DEV)
    call("rsu_mask_thin", hu.ptr(pt), TU.THRESHOLD, hu.ptr(lt), ITERS, None, hu.ptr(st), None, hu.ptr(info), hu.ptr(ws), N, S, S, hu.stream())
    _check_true(st, lt, info)
    # one image further is refused, before anything is launched
    assert lib().rsu_mask_thin(hu.ptr(pt), TU.THRESHOLD, hu.ptr(lt), ITERS, None, hu.ptr(st), None, hu.ptr(info), hu.ptr(ws), N + 1, S, S,
                               hu.stream()) == -7
    lu.done(pt, lt, ws, st, info)


def test_both_outputs_and_acc_at_the_limit():
    pt, lt, ws = _batch()
    _, _, (want_p, _, want_c, _) = _live()
    st = torch.full((N, S, S), -7, dtype=torch.int64, device=hu.DEV)
    sp = torch.full((N, S, S), float("nan"), dtype=torch.float32, device=hu.DEV)
    info = torch.full((N, 2), -7, dtype=torch.int32, device=hu.DEV)
    acc = torch.zeros(4, dtype=torch.int64, device=hu.DEV)
    call("rsu_mask_thin", hu.ptr(pt), TU.THRESHOLD, hu.ptr(lt), ITERS, hu.ptr(sp), hu.ptr(st), hu.ptr(acc), hu.ptr(info), hu.ptr(ws), N, S, S,
         hu.stream())
    _check_true(st, lt, info)
    for n, k in ((0, 0), (N - 1, 1)):
        assert sp[n].cpu().numpy().tobytes() == want_p[k].tobytes(), n
    assert not bool(sp[1:N - 1].view(torch.int32).any().item())     # +0.0 everywhere: the ignored images have no prediction
    assert want_c.min() > 1000 and np.array_equal(acc.cpu().numpy(), want_c)
    lu.done(pt, lt, ws, st, sp, info, acc)
