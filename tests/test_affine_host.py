"""The one-launch batch loader without a GPU: hostio.affine_patches (the numpy float32 statement of include/rsu.h rsu_affine_patches, the
yardstick of tests/test_gpu_affine.py) against independent statements of the rule -- the pool's plain window, d4_apply, a float64 bilinear
interpolation over np.pad(..., "symmetric") -- and pool.affine_draw, the flags and the ABI's argument checks."""
import ctypes
import glob
import itertools
import math
import os

import numpy as np
import pytest
import torch

from road_segmentation_unet_amd import hostio, pool
from road_segmentation_unet_amd.cli import parse_options
from road_segmentation_unet_amd.model import EXTRA_FLAG_DEFS, FLAG_DEFS, Options
from tests.affine_util import (D4_OPS, DYADIC, GEOMS, STRIDE, abi_call, abi_cases, bilinear64, make_images, rec, rotation_records,
                               value_bound)

@pytest.mark.parametrize("Hl,offset,S,P", GEOMS)
def test_identity_records_return_the_pools_window(Hl, offset, S, P):
    ext, lab = make_images(3, Hl, offset)
    pp = pool.PatchPool(ext, lab, S, P, STRIDE[S])
    idx = [0, 1, len(pp) // 2, len(pp) - 1, 7]
    gx, gy = pp.gather(idx)
    recs = []
    for k in idx:
        n, x0, y0 = pp.locate(k)
        recs.append(rec(n, y0 + (S - 1) / 2.0, x0 + (S - 1) / 2.0, np.eye(2)))
    x, y = hostio.affine_patches(ext, lab, recs, S, P)
    assert x.dtype == np.float32 and y.dtype == np.int64 and x.shape == (5, S, S, 3) and y.shape == (5, P, P)
    assert np.array_equal(x.view(np.int32), gx.view(np.int32))
    assert np.array_equal(y, gy.astype(np.int64))


@pytest.mark.parametrize("Hl,offset,S,P", GEOMS)
def test_every_d4_draw_equals_d4_apply(Hl, offset, S, P):
    ext, lab = make_images(2, Hl, offset, seed=1)
    pp = pool.PatchPool(ext, lab, S, P, STRIDE[S])
    k = 3
    n, x0, y0 = pp.locate(k)
    gx, gy = pp.gather([k])
    seen = set()
    for op in D4_OPS:
        D = pool.d4_matrix(op)
        x, y = hostio.affine_patches(ext, lab, [rec(n, y0 + (S - 1) / 2.0, x0 + (S - 1) / 2.0, D)], S, P)
        wx = pool.d4_apply(torch.from_numpy(gx[0]), op).contiguous().numpy()
        wy = pool.d4_apply(torch.from_numpy(gy[0]), op).contiguous().numpy()
        assert np.array_equal(x[0].view(np.int32), wx.view(np.int32)), op
        assert np.array_equal(y[0], wy.astype(np.int64)), op
        seen.add(x[0].tobytes())
    assert len(seen) == 8          # the image is not symmetric: the 32 draws give the 8 distinct elements of D4


@pytest.mark.parametrize("Hl,offset,S,P", GEOMS)
def test_dyadic_matrices_equal_the_float64_restatement(Hl, offset, S, P):
    """0.5 I and a shear by 1/4: every coordinate and every fraction is exact in float32, so labels match exactly and values to 1e-6"""
    ext, lab = make_images(3, Hl, offset, seed=2)
    c = offset + (Hl - 1) / 2.0
    recs = [rec(i % 3, cy, cx, M) for i, (M, (cy, cx)) in enumerate(itertools.product(
        DYADIC, [(c, c), (offset - 0.5, offset - 0.5), (offset + Hl - 0.5, offset + 2.0), (c + 0.25, c - 0.75)]))]
    x, y = hostio.affine_patches(ext, lab, recs, S, P)
    rx, ry = bilinear64(ext, lab, recs, S, P)
    assert float(np.abs(x - rx).max()) <= 1e-6
    assert np.array_equal(y, (ry >= 0.5).astype(np.int64))
    assert 0 < int(y.sum()) < y.size


@pytest.mark.parametrize("Hl,offset,S,P", GEOMS)
def test_general_rotations_stay_within_the_derived_bound(Hl, offset, S, P):
    ext, lab = make_images(3, Hl, offset, seed=3)
    recs = rotation_records(np.random.RandomState(11), 24, 3, Hl, offset)
    x, y = hostio.affine_patches(ext, lab, recs, S, P)
    rx, _ = bilinear64(ext, lab, recs, S, P)
    err, bound = float(np.abs(x - rx).max()), value_bound(ext, lab, recs, S)
    print("max |float32 - float64| %.3e, bound %.3e" % (err, bound))
    assert err <= bound
    assert set(np.unique(y)) <= {0, 1} and 0 < int(y.sum()) < y.size
    orig = ext[:, offset:offset + Hl, offset:offset + Hl]
    assert float(x.min()) >= float(orig.min()) and float(x.max()) <= float(orig.max())     # bilinear convexity


def test_sampling_three_widths_outside_crosses_reflection_periods():
    """scale 0.25 (|M| = 4) and a centre three image widths outside: tap indices run over several periods of 2 Hl on both sides of 0"""
    Hl, offset, S, P = 20, 4, 12, 4
    ext, lab = make_images(2, Hl, offset, seed=4)
    recs = [rec(0, offset - 3.0 * Hl, offset + 4.0 * Hl - 0.5, 4.0 * np.eye(2)), rec(1, offset + 3.5 * Hl, offset - 2.25 * Hl, [[0, -4.0], [4.0, 0]])]
    periods = set()
    for r in hostio.affine_records(recs):
        d = np.arange(S) - (S - 1) / 2.0
        sy = (float(r["cy"]) - offset) + float(r["m00"]) * d[:, None] + float(r["m01"]) * d[None, :]
        periods |= set(np.floor(sy / (2 * Hl)).astype(int).ravel())
    assert len(periods) >= 3 and min(periods) < 0 < max(periods)
    x, y = hostio.affine_patches(ext, lab, recs, S, P)
    rx, ry = bilinear64(ext, lab, recs, S, P)
    assert float(np.abs(x - rx).max()) <= 1e-6                        # (dyadic again: exact coordinates)
    assert np.array_equal(y, (ry >= 0.5).astype(np.int64))


def test_mirror_refuses_what_the_abi_refuses():
    ext, lab = make_images(2, 20, 4)
    good = rec(0, 9.5, 9.5, np.eye(2))
    hostio.affine_patches(ext, lab, [good], 12, 4)
    for bad in ([rec(2, 9.5, 9.5, np.eye(2))], [rec(-1, 9.5, 9.5, np.eye(2))], [rec(0, float("nan"), 9.5, np.eye(2))],
                [rec(0, 9.5, 9.5, 65.0 * np.eye(2))], [rec(0, 9.5, 9.5, [[1, float("inf")], [0, 1]])], []):
        with pytest.raises(ValueError):
            hostio.affine_patches(ext, lab, bad, 12, 4)
    for S, P in ((12, 5), (4, 12), (10, 4), (14, 4)):
        with pytest.raises(ValueError):
            hostio.affine_patches(ext, lab, [good], S, P)


# ------------------------------------------------------------------------------------------- draws
def test_affine_draw_with_d4_alone_consumes_the_stream_as_d4_draw_does():
    a, b = np.random.RandomState(5), np.random.RandomState(5)
    ops = pool.d4_draw(a, 7)
    M = pool.affine_draw(b, 7, rotation=0.0, scale=(1.0, 1.0), d4=True)
    assert M.dtype == np.float32 and M.shape == (7, 2, 2)
    assert a.random_sample() == b.random_sample()
    for m, op in zip(M, ops):
        assert np.array_equal(m, pool.d4_matrix(op).astype(np.float32))
    c = np.random.RandomState(5)
    assert np.array_equal(pool.affine_draw(c, 3), np.stack([np.eye(2, dtype=np.float32)] * 3))   # nothing on: nothing drawn
    assert c.random_sample() == np.random.RandomState(5).random_sample()


def test_affine_draw_is_deterministic_by_seed_and_stays_in_range():
    kw = dict(rotation=30.0, scale=(0.8, 1.25))
    A = pool.affine_draw(np.random.RandomState(3), 200, d4=False, **kw)
    assert np.array_equal(A, pool.affine_draw(np.random.RandomState(3), 200, d4=False, **kw))
    assert not np.array_equal(A, pool.affine_draw(np.random.RandomState(4), 200, d4=False, **kw))
    det = A[:, 0, 0].astype(np.float64) * A[:, 1, 1] - A[:, 0, 1].astype(np.float64) * A[:, 1, 0]
    s = 1.0 / np.sqrt(det)                                    # M = (1 / s) R(theta)
    theta = np.degrees(np.arctan2(A[:, 1, 0].astype(np.float64), A[:, 0, 0]))
    eps = 1e-5
    assert s.min() >= 0.8 - eps and s.max() <= 1.25 + eps and s.max() - s.min() > 0.3
    assert np.abs(theta).max() <= 30.0 + eps and theta.max() - theta.min() > 40.0
    assert np.allclose(A[:, 0, 0], A[:, 1, 1], atol=1e-6) and np.allclose(A[:, 0, 1], -A[:, 1, 0], atol=1e-6)
    # the order of the draws per sample: four D4 uniforms, the angle, the zoom
    rng = np.random.RandomState(8)
    B = pool.affine_draw(rng, 2, d4=True, **kw)
    u = np.random.RandomState(8).random_sample((2, 6))
    for j in range(2):
        op = (bool(u[j, 0] > 0.5), bool(u[j, 1] > 0.5), bool(u[j, 2] > 0.5), int(np.floor(u[j, 3] * 4)))
        th = math.radians((2.0 * u[j, 4] - 1.0) * 30.0)
        sc = math.exp(math.log(0.8) + u[j, 5] * (math.log(1.25) - math.log(0.8)))
        want = ((1.0 / sc) * np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])) @ pool.d4_matrix(op)
        assert np.array_equal(B[j], want.astype(np.float32))
    # rotation alone and zoom alone draw one uniform per sample
    for k in (dict(rotation=10.0), dict(scale=(0.5, 2.0))):
        r1, r2 = np.random.RandomState(1), np.random.RandomState(1)
        pool.affine_draw(r1, 5, **k)
        r2.random_sample((5, 1))
        assert r1.random_sample() == r2.random_sample()
    for bad in (dict(rotation=-1.0), dict(rotation=float("nan")), dict(scale=(2.0, 1.0)), dict(scale=(0.0, 1.0)), dict(scale=(1.0,)),
                dict(scale=(1.0, 65.0)), dict(scale=(1.0, float("inf")))):
        with pytest.raises(ValueError):
            pool.affine_draw(np.random.RandomState(0), 1, **bad)


def test_loader_flags_and_command_line():
    assert len(FLAG_DEFS) == 30                                            # the reference's flags stay the reference's
    defs = {d[0]: d for d in EXTRA_FLAG_DEFS}
    assert defs["random_rotation"][1:3] == (float, 0.0) and defs["random_scale"][1:3] == (str, "1,1")
    assert defs["one_launch_loader"][1:3] == (bool, False)
    o = Options()
    assert o.random_rotation == 0.0 and o.random_scale == (1.0, 1.0) and o.one_launch_loader is False
    o = parse_options(["--random_rotation=180", "--random_scale=0.8,1.25", "--one_launch_loader", "--d4_augmentation"])
    assert o.random_rotation == 180.0 and o.random_scale == (0.8, 1.25) and o.one_launch_loader is True and o.d4_augmentation is True
    assert parse_options(["--random_rotation", "0"]).random_rotation == 0.0
    assert parse_options(["--random_scale=2,2"]).random_scale == (2.0, 2.0)
    assert parse_options(["--noone_launch_loader"]).one_launch_loader is False
    assert Options(random_scale=(0.5, 2)).random_scale == (0.5, 2.0) and Options(random_rotation="15").random_rotation == 15.0
    nan, inf = float("nan"), float("inf")
    for bad in (-1.0, nan, inf, -inf, "x", None, True):
        with pytest.raises(ValueError):
            Options(random_rotation=bad)
    for bad in ("2,1", "1", "1,2,3", "nan,1", "1,inf", "0,1", "0.015625,1", "1,65", "-1,1", "a,b", "", None, 1.0, (1.0, nan)):
        with pytest.raises(ValueError):
            Options(random_scale=bad)
    for argv in (["--random_rotation=-5"], ["--random_rotation=nan"], ["--random_scale=2,1"], ["--random_scale=1.5"], ["--random_scale=1,inf"]):
        with pytest.raises(ValueError):
            parse_options(argv)
    # with the host pool the flags are refused, not ignored
    for argv in (["--random_rotation=30"], ["--random_scale=0.8,1.25"], ["--one_launch_loader"]):
        with pytest.raises(ValueError, match="nodevice_patch_pool"):
            parse_options(argv + ["--nodevice_patch_pool"])
    assert parse_options(["--nodevice_patch_pool", "--d4_augmentation"]).device_patch_pool is False   # (as before)


# ------------------------------------------------------------------------------------------- the ABI, on the host
def test_abi_refuses_bad_arguments_on_the_host():
    """every refused call returns from host code before anything is launched (no GPU is needed: the device pointers are never
    dereferenced)"""
    from road_segmentation_unet_amd import _lib
    L = _lib.lib()
    assert ctypes.sizeof(_lib.RsuAffine) == hostio.AFFINE_DTYPE.itemsize == 32 and _lib.AFFINE_MAX_LAUNCH == 32
    assert [n for n, _ in _lib.RsuAffine._fields_] == list(hostio.AFFINE_DTYPE.names)
    p = ctypes.c_void_p(4096)
    ok = dict(images=p, labels=p, x_out=p, labels_out=p, recs=[rec(0, 9.5, 9.5, np.eye(2))], nimg=3, He=28, Hl=20, S=12, P=4)
    for name, b in abi_cases():
        assert abi_call(L, dict(ok, **b)) == -22, name
    big = dict(ok, He=13400 + 8, Hl=13400, S=12, P=4)                       # one image of 2.15 GB
    assert abi_call(L, big) == _lib.E2BIG
    assert abi_call(L, dict(ok, He=7008, Hl=7000, S=6708, P=6700, recs=[rec(0, 9.5, 9.5, np.eye(2))] * 4)) == _lib.E2BIG   # x_out of 2.16 GB


def test_kernel_isa_has_no_fused_multiply_add():
    """hostio.affine_patches restates the kernel's float32 arithmetic operation by operation: the compiled kernel must round every
    multiply and add on its own. Reads the ISA the build keeps."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    isa = glob.glob(os.path.join(root, "road_segmentation_unet_amd", "csrc", "build", "affine_patches-hip-*gfx950.s"))
    assert isa, "build() keeps the ISA of every kernel file (-save-temps=obj)"
    text = open(isa[0]).read()
    for fused in ("v_fma_f32", "v_fmac_f32", "v_fmaak_f32", "v_fmamk_f32", "v_mad_f32", "v_mac_f32", "v_pk_fma_f32"):
        assert fused not in text, fused
    assert "v_mul_f32" in text and "v_floor_f32" in text
