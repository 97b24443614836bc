"""-m gpu: rsu_distance_hist with labels64 one image short of the 2-GiB limit -- 255 images of 1024 x 1024, 0x7f800000 bytes of labels, the
largest batch rsu_distance.h admits at the largest side -- and rsu_mask_distance on the same batch, checked on the host at the image that holds byte 2^30 of labels64 and on the device everywhere.

The kernels form every pixel's offset as image * H * W + y * W + x: whether that stays in range shows only when the last image ends just
below 2^31 bytes. The batch is periodic over tests/large_util.K mask pairs built on the device (tests/large_util.periodic); images are
independent, so the expected histogram is the host's histogram of each pattern times the number of images that carry it, and the
expected distances of any image are its pattern's. All comparisons are integer equality; no whole tensor comes to the host."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import distance_util as DU  # noqa: E402
from tests import hiputil as hu  # noqa: E402
from tests import large_util as lu  # noqa: E402
from road_segmentation_unet_amd import hostio  # noqa: E402
from road_segmentation_unet_amd._lib import call, lib  # noqa: E402

S = DU.MAX_SIDE
K = lu.K


@pytest.fixture(autouse=True)
def _large_test():
    lu.need_memory()
    yield
    lu.done()


def _patterns():
    """K pairs (prob float32, labels int64) [K, S, S]: truth of random blobs' density 0.02 to 0.05, the prediction the truth moved by a
    few pixels with specks added and removed, about 3 % of the labels ignored: distances of a few pixels, a few far ones"""
    rng = np.random.RandomState(41)
    true = np.stack([rng.random_sample((S, S)) < d for d in (0.02, 0.035, 0.05)])
    pred = np.stack([DU.shifted(true[k:k + 1], dy, dx)[0] for k, (dy, dx) in enumerate(((2, -1), (-3, 2), (1, 4)))])
    pred ^= rng.random_sample(pred.shape) < 0.002
    labels = true.astype(np.int64)
    labels[rng.random_sample(labels.shape) < 0.03] = -1
    prob = np.where(pred, np.float32(0.75), np.float32(0.25)).astype(np.float32)
    prob[:, ::7, ::5] = np.float32(DU.THRESHOLD)     # the threshold itself: inside
    prob[:, 3::7, ::5] = np.float32(np.nan)          # outside
    return prob, labels


def test_distance_hist_and_mask_distance_at_the_limit():
    N = lu.n_max(S * S * 8)
    assert N == 255 and N * S * S * 8 < lu.LIMIT <= (N + 1) * S * S * 8
    assert lib().rsu_distance_ws_bytes(N, S, S) == N * S * S * 4
    prob, labels = _patterns()
    mult = np.array([(N - k + K - 1) // K for k in range(K)], np.int64)
    want = np.zeros((2, DU.BINS), np.int64)
    for k in range(K):
        want += mult[k] * hostio.distance_hist(prob[k:k + 1], DU.THRESHOLD, labels[k:k + 1])
    assert want[0, 1:8].min() > 0 and want[1, 1:6].min() > 0 and want.sum() > 1 << 22
    pt, lt = lu.periodic(prob, N, torch.float32), lu.periodic(labels, N, torch.int64)
    ws = torch.full((N * S * S,), 0x7FA57FA5, dtype=torch.int32, device=hu.DEV)
    acc = DU.run_hist(pt, lt, (N, S, S), ws=ws)
    got = acc.cpu().numpy()
    assert np.array_equal(got, want), (got, want)
    # one image further is refused, before anything is launched
    assert lib().rsu_distance_hist(hu.ptr(pt), DU.THRESHOLD, hu.ptr(lt), hu.ptr(acc), hu.ptr(ws), N + 1, S, S, hu.stream()) == -7
    assert np.array_equal(acc.cpu().numpy(), want)
    # the exact distances over the whole batch; on the host those of the first image, of the one that holds byte 2^30 of labels64 (prob,
    # ws and the outputs, at 4 bytes per pixel, end below it), of its successor and of the last: their patterns'
    s = lu.straddler(S * S * 8)
    assert s == 128 and 0 < s < s + 1 < N - 1
    d2p = torch.full((N, S, S), -7, dtype=torch.int32, device=hu.DEV)
    d2t = torch.full((N, S, S), -7, dtype=torch.int32, device=hu.DEV)
    call("rsu_mask_distance", hu.ptr(pt), DU.THRESHOLD, hu.ptr(lt), hu.ptr(d2p), hu.ptr(d2t), hu.ptr(ws), N, S, S, hu.stream())
    for n in (0, s, s + 1, N - 1):
        wp, wt = hostio.mask_distance(prob[n % K:n % K + 1], DU.THRESHOLD, labels[n % K:n % K + 1])
        assert np.array_equal(d2p[n].cpu().numpy(), wp[0]) and np.array_equal(d2t[n].cpu().numpy(), wt[0]), n
    lu.assert_periodic_bits(d2p, "d2_pred")
    lu.assert_periodic_bits(d2t, "d2_true")
    lu.done(pt, lt, ws, d2p, d2t, acc)
