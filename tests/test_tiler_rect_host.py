"""No GPU: the tile grid of prediction on images of any size (hostio.tile_origins, rsu_tile_grid), the argument checks of the rect tiler
entries (they return before anything touches the device), and the host formats either side of it on H != W."""
import ctypes

import numpy as np
import pytest

from road_segmentation_unet_amd import hostio
from road_segmentation_unet_amd._lib import lib

from tests import rect_util as R

EINVAL = -22


def test_tile_origins_rule():
    assert hostio.tile_origins(8, 8, 5) == [0]
    assert hostio.tile_origins(388, 388, 1) == [0]
    for L, P, s in [(20, 8, 4), (44, 20, 12), (16, 16, 16), (604, 388, 12), (608, 388, 110), (9, 8, 1)]:
        assert (L - P) % s == 0
        assert hostio.tile_origins(L, P, s) == list(range(0, L - P + 1, s))
    assert hostio.tile_origins(31, 8, 5) == [0, 5, 10, 15, 20, 23]
    for L, P, s in [(9, 8, 16), (30, 20, 11), (400, 388, 110)]:
        assert s > L - P > 0
        assert hostio.tile_origins(L, P, s) == [0, L - P]
    assert hostio.tile_origins(400, 388, 110) == [0, 12]
    for bad in [(7, 8, 1), (8, 8, 0), (8, 0, 1)]:
        with pytest.raises(ValueError):
            hostio.tile_origins(*bad)
    with pytest.raises(ValueError, match="patch_size=388"):
        hostio.tile_origins(300, 388, 12)


def test_tile_grid_abi_agrees_on_a_sweep():
    L_ = lib()
    ny, nx = ctypes.c_int(-1), ctypes.c_int(-1)
    for P in (1, 3, 8):
        for s in (1, 2, 3, 5, 8, 13):
            for L in range(P, P + 30):
                want = hostio.tile_origins(L, P, s)
                assert want == R.origins(L, P, s)
                assert want[0] == 0 and want[-1] == L - P and all(b > a for a, b in zip(want, want[1:]))
                W = P + (L * 7) % 11
                assert L_.rsu_tile_grid(L, W, P, s, ctypes.byref(ny), ctypes.byref(nx)) == 0
                assert (ny.value, nx.value) == (len(want), len(hostio.tile_origins(W, P, s))), (L, W, P, s)
    for H, W, P, s in [(7, 9, 8, 1), (9, 7, 8, 1), (9, 9, 8, 0), (9, 9, 0, 1)]:
        assert L_.rsu_tile_grid(H, W, P, s, ctypes.byref(ny), ctypes.byref(nx)) == EINVAL
    assert L_.rsu_tile_grid(9, 9, 8, 1, None, ctypes.byref(nx)) == EINVAL
    assert L_.rsu_tile_grid(9, 9, 8, 1, ctypes.byref(ny), None) == EINVAL


def test_rect_entries_refuse_bad_arguments_before_the_device():
    """every refused call returns RSU_EINVAL on a machine without a GPU: the pointers are dummies that are never followed"""
    L_ = lib()
    a, b, c = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000), ctypes.c_void_p(0x3000)
    # (nimg, H, W, S, P, stride, t0, ntiles); the grid of 23 x 31 at P = 8, stride 5 is 4 x 6: 48 tiles in two images
    good = dict(nimg=2, H=23, W=31, S=12, P=8, stride=5, t0=0, ntiles=48)
    bad = [dict(nimg=0), dict(nimg=-1), dict(H=7), dict(W=7), dict(P=13, S=12), dict(S=11), dict(S=6), dict(stride=0), dict(stride=-3),
           dict(t0=-1), dict(ntiles=0), dict(ntiles=49), dict(t0=1), dict(t0=48, ntiles=1)]

    def extract(imgs, tiles, g):
        return L_.rsu_extract_tiles_rect(imgs, tiles, g["nimg"], g["H"], g["W"], g["S"], g["P"], g["stride"], g["t0"], g["ntiles"], None)

    def add(prob, acc, hits, g):
        return L_.rsu_overlap_add_rect(prob, acc, hits, g["nimg"], g["H"], g["W"], g["P"], g["stride"], g["t0"], g["ntiles"], None)
    for change in bad:   # (H=7, W=7: P > H, P > W)
        assert extract(a, b, dict(good, **change)) == EINVAL, change
    for change in [ch for ch in bad if "S" not in ch]:
        assert add(a, b, c, dict(good, **change)) == EINVAL, change
    assert extract(None, b, good) == EINVAL and extract(a, None, good) == EINVAL
    assert add(None, b, c, good) == EINVAL and add(a, None, c, good) == EINVAL and add(a, b, None, good) == EINVAL

    def quant(m, o, nimg=2, H=40, W=56, ps=16):
        return L_.rsu_quantize_mask_rect(m, o, nimg, H, W, ps, 0.25, None)
    assert quant(None, b) == EINVAL and quant(a, None) == EINVAL
    for kw in [dict(nimg=0), dict(H=0), dict(W=0), dict(ps=0), dict(ps=65)]:
        assert quant(a, a, **kw) == EINVAL, kw


def test_host_quantize_mask_on_a_rectangle():
    rng = np.random.RandomState(5)
    m = rng.rand(2, 40, 56, 1)
    m[0, :16, :16] = 0.6    # a block far above the threshold, one far below, the rest near it
    m[1, 32:, 48:] = 0.1
    got = hostio.quantize_mask(m, 0.25, 16)
    assert got.shape == m.shape
    want = np.empty_like(m)
    for k in range(2):
        for y in range(0, 40, 16):        # the last row of blocks holds 8 of its 16 rows
            for x in range(0, 56, 16):    # the last column of blocks holds 8 of its 16 columns
                blk = m[k, y:min(y + 16, 40), x:min(x + 16, 56), 0]
                want[k, y:y + 16, x:x + 16, 0] = float((blk >= 0.5).sum() / blk.size > 0.25)
    np.testing.assert_array_equal(got, want)
    assert 0 < want.mean() < 1


def test_submission_rows_on_a_rectangle():
    rng = np.random.RandomState(6)
    masks = (rng.rand(2, 32, 48) < 0.3).astype(np.float64)
    masks[0, 16:, :16] = 1.0
    masks[1, :16, 32:] = 0.0
    rows = hostio.submission_rows(masks, 16)
    assert len(rows) == 2 * 2 * 3
    want = []
    for k in range(2):
        for j in range(3):        # x outer
            for i in range(2):
                lab = int(masks[k, 16 * i:16 * i + 16, 16 * j:16 * j + 16].mean() > 0.25)
                want.append("%03d_%d_%d,%d" % (k + 1, 16 * j, 16 * i, lab))
    assert rows == want
    assert rows[1] == "001_0_16,1" and rows[10] == "002_32_0,0"
    assert hostio.submission_rows(masks[..., None], 16) == rows
    with pytest.raises(ValueError):
        hostio.submission_rows(np.zeros((1, 40, 48)), 16)
    with pytest.raises(ValueError):
        hostio.submission_rows(np.zeros((1, 48, 40)), 16)


def test_load_refuses_a_directory_of_mixed_shapes(tmp_path):
    from PIL import Image
    Image.fromarray(np.zeros((48, 64, 3), np.uint8)).save(tmp_path / "a.png")
    Image.fromarray(np.zeros((48, 64, 3), np.uint8)).save(tmp_path / "b.png")
    assert hostio.load(str(tmp_path)).shape == (2, 48, 64, 3)
    Image.fromarray(np.zeros((64, 48, 3), np.uint8)).save(tmp_path / "c.png")
    with pytest.raises(ValueError, match="differ in shape"):
        hostio.load(str(tmp_path))
