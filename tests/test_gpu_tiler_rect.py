"""-m gpu: the tiler entries for images of any size (rsu_extract_tiles_rect, rsu_overlap_add_rect, rsu_quantize_mask_rect) against the
numpy statement of the tile rule (tests/rect_util.py) and, where the square entries accept the input, against those entries bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from road_segmentation_unet_amd import hostio  # noqa: E402
from road_segmentation_unet_amd._lib import call  # noqa: E402
from tests import hiputil as hu  # noqa: E402
from tests import rect_util as R  # noqa: E402


def _extract_rect(idev, nimg, H, W, S, P, stride, nt):
    """all nt tiles in two calls split at nt // 2"""
    tiles = torch.zeros((nt, S, S, 3), dtype=torch.float32, device=hu.DEV)
    half = nt // 2
    if half:
        call("rsu_extract_tiles_rect", hu.ptr(idev), hu.ptr(tiles), nimg, H, W, S, P, stride, 0, half, hu.stream())
    call("rsu_extract_tiles_rect", hu.ptr(idev), hu.ptr(tiles[half:]), nimg, H, W, S, P, stride, half, nt - half, hu.stream())
    return tiles


def _overlap_rect(pdev, nimg, H, W, P, stride, nt):
    acc = torch.zeros((nimg, H, W), dtype=torch.float32, device=hu.DEV)
    hits = torch.zeros((nimg, H, W), dtype=torch.float32, device=hu.DEV)
    half = nt // 2
    if half:
        call("rsu_overlap_add_rect", hu.ptr(pdev), hu.ptr(acc), hu.ptr(hits), nimg, H, W, P, stride, 0, half, hu.stream())
    call("rsu_overlap_add_rect", hu.ptr(pdev[half:]), hu.ptr(acc), hu.ptr(hits), nimg, H, W, P, stride, half, nt - half, hu.stream())
    return acc, hits


@pytest.mark.parametrize("nimg,H,W,P,S,stride", [
    (2, 23, 31, 8, 12, 5),      # y covered exactly, x with a clamped last tile
    (1, 9, 8, 8, 12, 16),       # stride above P: two tiles one pixel apart on y, one tile on x
    (2, 8, 11, 8, 40, 3),       # a border of 16 on images 8 x 11: two reflections
    (3, 44, 44, 20, 60, 12),    # square, covered exactly
])
def test_rect_tiler_against_the_rule(nimg, H, W, P, S, stride):
    rng = np.random.RandomState(H * 100 + W)
    imgs = rng.rand(nimg, H, W, 3).astype(np.float32)
    nt = len(R.tile_list(nimg, H, W, P, stride))
    assert nt == nimg * len(hostio.tile_origins(W, P, stride)) * len(hostio.tile_origins(H, P, stride))
    tiles = _extract_rect(hu.dev_f32(imgs), nimg, H, W, S, P, stride, nt)
    np.testing.assert_array_equal(hu.host(tiles), R.extract(imgs, S, P, stride))   # bit-exact: pure data movement
    prob = rng.rand(nt, P, P).astype(np.float32)
    acc, hits = _overlap_rect(hu.dev_f32(prob), nimg, H, W, P, stride, nt)
    out = torch.zeros_like(acc)
    call("rsu_overlap_finish", hu.ptr(acc), hu.ptr(hits), hu.ptr(out), acc.numel(), hu.stream())
    refm, refh = R.overlap(prob, nimg, H, W, stride)
    assert refh.min() >= 1
    np.testing.assert_array_equal(hu.host(hits), refh.astype(np.float32))
    np.testing.assert_allclose(hu.host(out), refm, rtol=2e-6, atol=1e-7)   # float accumulator against a float64 reference


@pytest.mark.parametrize("H,P,S,stride,nimg", [(20, 8, 12, 4, 2), (44, 20, 60, 12, 3), (16, 16, 24, 16, 1)])
def test_rect_tiler_gives_the_square_entries_bits(H, P, S, stride, nimg):
    rng = np.random.RandomState(H)
    imgs = rng.rand(nimg, H, H, 3).astype(np.float32)
    pps = (H - P) // stride + 1
    nt = nimg * pps * pps
    idev = hu.dev_f32(imgs)
    tiles = _extract_rect(idev, nimg, H, H, S, P, stride, nt)
    old = torch.zeros_like(tiles)
    half = nt // 2
    if half:
        call("rsu_extract_tiles", hu.ptr(idev), hu.ptr(old), nimg, H, S, P, stride, 0, half, hu.stream())
    call("rsu_extract_tiles", hu.ptr(idev), hu.ptr(old[half:]), nimg, H, S, P, stride, half, nt - half, hu.stream())
    torch.cuda.synchronize()
    assert torch.equal(tiles, old)
    pdev = hu.dev_f32(rng.rand(nt, P, P).astype(np.float32))
    acc, hits = _overlap_rect(pdev, nimg, H, H, P, stride, nt)
    acc0, hits0 = torch.zeros_like(acc), torch.zeros_like(hits)
    if half:
        call("rsu_overlap_add", hu.ptr(pdev), hu.ptr(acc0), hu.ptr(hits0), nimg, H, P, stride, 0, half, hu.stream())
    call("rsu_overlap_add", hu.ptr(pdev[half:]), hu.ptr(acc0), hu.ptr(hits0), nimg, H, P, stride, half, nt - half, hu.stream())
    torch.cuda.synchronize()
    assert torch.equal(acc, acc0) and torch.equal(hits, hits0)
    assert float(hits.min()) >= 1


def _mask(rng, n, H, W):
    m = rng.rand(n, H, W, 1).astype(np.float32)
    m[0, :16, :16] = 0.6    # a block far above the threshold, one far below, the rest near it
    m[-1, 32:, 32:] = 0.1
    return m


def test_quantize_mask_rect():
    rng = np.random.RandomState(9)
    m = _mask(rng, 2, 40, 56)   # the last row and column of blocks hold 8 of their 16 pixels
    want = hostio.quantize_mask(m, 0.25, 16)[..., 0]
    src = hu.dev_f32(m[..., 0])
    out = torch.full_like(src, -1.0)
    call("rsu_quantize_mask_rect", hu.ptr(src), hu.ptr(out), 2, 40, 56, 16, 0.25, hu.stream())
    np.testing.assert_array_equal(hu.host(out), want)
    np.testing.assert_array_equal(hu.host(src), m[..., 0])
    call("rsu_quantize_mask_rect", hu.ptr(src), hu.ptr(src), 2, 40, 56, 16, 0.25, hu.stream())   # in place
    np.testing.assert_array_equal(hu.host(src), want)
    assert 0 < want.mean() < 1
    sq = hu.dev_f32(_mask(rng, 2, 40, 40)[..., 0])
    a, b = torch.empty_like(sq), torch.empty_like(sq)
    call("rsu_quantize_mask_rect", hu.ptr(sq), hu.ptr(a), 2, 40, 40, 16, 0.25, hu.stream())
    call("rsu_quantize_mask", hu.ptr(sq), hu.ptr(b), 2, 40, 16, 0.25, hu.stream())
    torch.cuda.synchronize()
    assert torch.equal(a, b)
