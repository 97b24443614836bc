"""-m gpu: rsu_skeleton_graph with labels64 and the *_true outputs one image short of the 2-GiB limit -- 255 images of 1024 x 1024, 0x7f800000
bytes each, the largest batch rsu_graph.h admits at the largest side.

The kernels form every pixel's offset as image * H * W + y * W + x and every plane word's as (image * 2 + side) * H * Wq + y * Wq + xw:
whether they stay in range shows only when the last image ends just below 2^31 bytes. Only the first and the last image carry masks of the
bank (sparse noise and ragged blobs: pruning has branches to take, and the host is spared the thinning of four 1024 x 1024 masks), and
only those are held to hostio.skeleton_graph, byte for byte; every other image is ignored altogether (labels -1 under a probability above the threshold), and a reduction on the device asserts that its out_true is its
labels64 and its out_pred empty. min_branch R + 1: the second delete and the second regrow launch run. First the pruned masks in place,
as evaluate() calls the entry; then the junction outputs with acc. No whole tensor comes to the host."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import graph_util as GU  # noqa: E402
from tests import hiputil as hu  # noqa: E402
from tests import large_util as lu  # noqa: E402
from tests import thin_util as TU  # noqa: E402
from road_segmentation_unet_amd import hostio  # noqa: E402
from road_segmentation_unet_amd._lib import call, lib  # noqa: E402

S = GU.MAX_SIDE
BRANCH = GU.R + 1
N = 255
LIVE = ((0, 0), (N - 1, 1))


@pytest.fixture(autouse=True)
def _large_test():
    lu.need_memory()
    yield
    lu.done()


@functools.lru_cache(maxsize=None)
def _live():
    """(prob float32, labels int64) [2, S, S] of the first and the last image and hostio.skeleton_graph of them: computed once"""
    pred = np.stack([TU.masks("rand0.3", (1, S, S))[0], TU.masks("smooth1.5", (1, S, S))[0]])
    true = np.stack([TU.masks("smooth3", (1, S, S))[0], TU.masks("rand0.45", (1, S, S))[0]])
    labels = true.astype(np.int64)
    labels[:, ::11, ::13] = -1
    prob = np.where(pred, np.float32(0.75), np.float32(0.25)).astype(np.float32)
    prob[:, ::7, ::5] = np.float32(GU.THRESHOLD)     # the threshold itself: inside
    prob[:, 3::7, ::5] = np.float32(np.nan)          # outside
    return prob, labels, hostio.skeleton_graph(prob, GU.THRESHOLD, labels, BRANCH)


def _batch():
    prob, labels, _ = _live()
    pt = torch.full((N, S, S), 0.75, dtype=torch.float32, device=hu.DEV)
    lt = torch.full((N, S, S), -1, dtype=torch.int64, device=hu.DEV)
    for n, k in LIVE:
        pt[n].copy_(torch.from_numpy(prob[k]))
        lt[n].copy_(torch.from_numpy(labels[k]))
    need = int(lib().rsu_graph_ws_bytes(N, S, S, BRANCH))
    assert need > 0
    ws = torch.full((need // 8,), 0x7FA57FA57FA57FA5, dtype=torch.int64, device=hu.DEV)
    return pt, lt, ws


def _check(got_f, got_i, want_f, want_i):
    """the live images byte for byte; the ignored ones: the int64 output all -1, the float32 one all +0.0"""
    for n, k in LIVE:
        assert got_f[n].cpu().numpy().tobytes() == want_f[k].tobytes(), n
        assert got_i[n].cpu().numpy().tobytes() == want_i[k].tobytes(), n
    for n0 in range(1, N - 1, 32):
        n1 = min(n0 + 32, N - 1)
        assert bool((got_i[n0:n1] == -1).all().item()), (n0, n1)
        assert not bool(got_f[n0:n1].view(torch.int32).any().item()), (n0, n1)


def test_pruned_in_place_at_the_limit():
    assert N == lu.n_max(S * S * 8) and N * S * S * 8 < lu.LIMIT <= (N + 1) * S * S * 8
    pt, lt, ws = _batch()
    _, _, (want_p, want_t, _, _, want_c) = _live()
    assert want_c[0] < (_live()[0] >= GU.THRESHOLD).sum()     # (pruning takes pixels)
    acc = torch.zeros(8, dtype=torch.int64, device=hu.DEV)
    call("rsu_skeleton_graph", hu.ptr(pt), GU.THRESHOLD, hu.ptr(lt), BRANCH, hu.ptr(pt), hu.ptr(lt), None, None, hu.ptr(acc), hu.ptr(ws), N, S, S,
         hu.stream())
    _check(pt, lt, want_p, want_t)
    assert want_c[[0, 1, 3, 4, 5, 7]].min() > 100 and np.array_equal(acc.cpu().numpy(), want_c)
    # one image further is refused, before anything is launched
    assert lib().rsu_skeleton_graph(hu.ptr(pt), GU.THRESHOLD, hu.ptr(lt), BRANCH, hu.ptr(pt), hu.ptr(lt), None, None, hu.ptr(acc), hu.ptr(ws),
                                    N + 1, S, S, hu.stream()) == -7
    lu.done(pt, lt, ws, acc)


def test_junction_outputs_and_acc_at_the_limit():
    pt, lt, ws = _batch()
    _, _, (_, _, want_jp, want_jt, want_c) = _live()
    jp = torch.full((N, S, S), float("nan"), dtype=torch.float32, device=hu.DEV)
    jt = torch.full((N, S, S), -7, dtype=torch.int64, device=hu.DEV)
    acc = torch.zeros(8, dtype=torch.int64, device=hu.DEV)
    call("rsu_skeleton_graph", hu.ptr(pt), GU.THRESHOLD, hu.ptr(lt), BRANCH, None, None, hu.ptr(jp), hu.ptr(jt), hu.ptr(acc), hu.ptr(ws), N, S, S,
         hu.stream())
    _check(jp, jt, want_jp, want_jt)
    assert np.array_equal(acc.cpu().numpy(), want_c)
    lu.done(pt, lt, ws, jp, jt, acc)
