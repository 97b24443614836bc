"""Elastic deformation in the one-launch loader without a GPU: hostio.elastic_lattice, elastic_field and elastic_patches (the numpy float32
statement of include/rsu.h rsu_elastic_patches, the yardstick of tests/test_gpu_elastic.py) against independent statements of the rule --
hostio.affine_patches at alpha = 0, a constant lattice, a float64 spline -- and pool.elastic_draw, the flag and the ABI's argument checks."""
import ctypes

import numpy as np
import pytest

from road_segmentation_unet_amd import hostio, pool
from road_segmentation_unet_amd.cli import parse_options
from road_segmentation_unet_amd.model import EXTRA_FLAG_DEFS, FLAG_DEFS, Options, parse_elastic_deformation
from tests import affine_util as au
from tests import elastic_util as eu


@pytest.mark.parametrize("Hl,offset,S,P", eu.GEOMS)
def test_alpha_zero_returns_the_affine_loaders_bits(Hl, offset, S, P):
    """on the loader's own bank (tests/test_gpu_affine.py _case), under every grid and with keys that would matter if alpha did"""
    ext, lab, arecs, hx, hy = eu.affine_case(Hl, offset, S, P)
    assert len(arecs) == 51
    for G in eu.GRIDS:
        keys = np.random.RandomState(G).randint(0, 2 ** 32, size=len(arecs))
        x, y = hostio.elastic_patches(ext, lab, eu.elastic_of(arecs, 0.0, keys, G), S, P)
        assert x.dtype == np.float32 and y.dtype == np.int64
        assert np.array_equal(x.view(np.int32), hx.view(np.int32)) and np.array_equal(y, hy), G
    assert not hostio.elastic_field(hostio.elastic_lattice(77, 0.0, 3), S).any()          # u is zero, exactly


def test_weights_are_a_partition_of_unity_and_a_constant_lattice_gives_that_constant():
    f = np.random.RandomState(1).random_sample(1000).astype(np.float32)
    f[:3] = (0.0, 0.5, np.nextafter(np.float32(1.0), np.float32(0.0)))
    w = hostio.elastic_weights(f)
    assert w.dtype == np.float32 and w.shape == (4, 1000) and float(w.min()) >= 0.0
    total = ((w[0] + w[1]) + w[2]) + w[3]
    worst = float(np.abs(total.astype(np.float64) - 1.0).max())
    print("|sum of the four weights - 1| <= %.3e on 1000 fractions" % worst)
    assert worst <= 2.0 * 2.0 ** -23                                                       # 2 ulp of 1
    exact = np.stack([(1 - f.astype(np.float64)) ** 3, 3 * f.astype(np.float64) ** 3 - 6 * f.astype(np.float64) ** 2 + 4,
                      -3 * f.astype(np.float64) ** 3 + 3 * f.astype(np.float64) ** 2 + 3 * f.astype(np.float64) + 1, f.astype(np.float64) ** 3]) / 6.0
    werr = float(np.abs(w - exact).max())
    print("|weight - exact weight| <= %.3e, bound %.3e" % (werr, eu.weight_bound()))
    assert werr <= eu.weight_bound()
    for G in (1, 3, 4, 16):
        for c in (2.5, -13.88):
            for S in (11, 12, 20):
                lat = np.full((G + 3, G + 3, 2), c, np.float32)
                u = hostio.elastic_field(lat, S)
                assert u.shape == (2, S, S) and u.dtype == np.float32
                # no coordinate term: whatever cell and fraction a pixel gets, the exact field is c
                assert float(np.abs(u.astype(np.float64) - np.float64(np.float32(c))).max()) <= eu.field_bound(0.0, 0, cmax=abs(c)), (G, c, S)


@pytest.mark.parametrize("Hl,offset,S,P", eu.GEOMS)
def test_label_field_is_the_window_fields_centre_crop(Hl, offset, S, P):
    """an image whose every channel is its label mask: the label patch equals the thresholded centre crop of the input window under
    every record -- labels see the field at (i + offset, j + offset), by the same float operations -- and moving the crop by one pixel
    breaks it"""
    ext, lab, recs, _, _ = eu.case(Hl, offset, S, P)
    img = hostio.mirror_border(np.repeat(lab[..., None].astype(np.float32), 3, axis=3), offset)
    sub = recs[::7]
    x, y = hostio.elastic_patches(img, lab, sub, S, P)
    assert np.array_equal((x[:, offset:offset + P, offset:offset + P, 0] >= np.float32(0.5)).astype(np.int64), y)
    assert not np.array_equal((x[:, offset - 1:offset - 1 + P, offset:offset + P, 0] >= np.float32(0.5)).astype(np.int64), y)
    # and directly: the field of a label patch, formed from the label pixel's own window index, is the crop, bit for bit
    lat = hostio.elastic_lattice(99, 4.0, 3)
    u = hostio.elastic_field(lat, S)
    k, w = hostio._elastic_axis(S, 3)
    kl, wl = k[offset:offset + P], w[:, offset:offset + P]
    for axis in range(2):
        c = lat[:, :, axis]
        row = [((wl[0][None, :] * c[kl[:, None] + a, kl[None, :]] + wl[1][None, :] * c[kl[:, None] + a, kl[None, :] + 1])
                + wl[2][None, :] * c[kl[:, None] + a, kl[None, :] + 2]) + wl[3][None, :] * c[kl[:, None] + a, kl[None, :] + 3] for a in range(4)]
        ul = ((wl[0][:, None] * row[0] + wl[1][:, None] * row[1]) + wl[2][:, None] * row[2]) + wl[3][:, None] * row[3]
        assert np.array_equal(ul.view(np.int32), u[axis, offset:offset + P, offset:offset + P].view(np.int32))


def test_float32_field_stays_within_the_derived_bound_of_the_float64_spline():
    """eu.field_bound: (50 + 8 G) 2^-24 * 3.47 alpha, from the count of roundings (its docstring holds the derivation)"""
    keys = np.random.RandomState(3).randint(0, 2 ** 32, size=6)
    for G in (1, 3, 4, 16):
        for alpha in (0.75, 4.0, 64.0):
            for S in (11, 12, 20, 92):
                for key in keys:
                    lat = hostio.elastic_lattice(key, alpha, G)
                    assert lat.shape == (G + 3, G + 3, 2) and lat.dtype == np.float32 and float(np.abs(lat).max()) <= eu.MAX_G * alpha
                    u = hostio.elastic_field(lat, S)
                    err, bound = float(np.abs(u - eu.field64(lat, S)).max()), eu.field_bound(alpha, G)
                    assert err <= bound, (G, alpha, S, key, err, bound)
                    assert float(np.abs(u).max()) <= eu.MAX_G * alpha                      # a convex combination of the lattice
    lat = hostio.elastic_lattice(keys[0], 4.0, 16)
    print("G 16, alpha 4, S 92: max |float32 - float64| %.3e, bound %.3e"
          % (float(np.abs(hostio.elastic_field(lat, 92) - eu.field64(lat, 92)).max()), eu.field_bound(4.0, 16)))
    # the field is smooth: neighbouring pixels differ by at most the spline's slope, 2 C per cell, G / S cells per pixel
    u = hostio.elastic_field(hostio.elastic_lattice(keys[1], 4.0, 3), 92)
    assert float(np.abs(np.diff(u, axis=1)).max()) <= 2 * eu.MAX_G * 4.0 * 3 / 92 and float(np.abs(np.diff(u, axis=2)).max()) <= 2 * eu.MAX_G * 4.0 * 3 / 92
    assert float(u.std()) < 4.0                                                             # smaller than the control points' deviation


def test_lattice_statistics_over_64_keys():
    keys = np.random.RandomState(5).randint(0, 2 ** 32, size=64)
    v = np.concatenate([hostio.elastic_lattice(k, 1.0, 4).ravel() for k in keys]).astype(np.float64)
    assert v.size == 6272
    print("lattice values over 64 keys: mean %+.4f, deviation %.4f, max |v| %.3f" % (v.mean(), v.std(), np.abs(v).max()))
    assert abs(v.mean()) <= 5.0 / np.sqrt(6272.0)
    assert abs(v.std() - 1.0) <= 5.0 / np.sqrt(2.0 * 6272.0)
    assert np.abs(v).max() <= 3.47
    # the element index is (a * 32 + b) * 2 + axis under the jitter's hash, and alpha scales it with one rounding
    a, b, axis, key = 5, 2, 1, int(keys[0])
    n = hostio.jitter_noise_int(key, (a * 32 + b) * 2 + axis + 1)[-1]
    g = (np.float32(n) - np.float32(131070.0)) * hostio.JITTER_NOISE_SCALE
    assert hostio.elastic_lattice(key, 1.0, 4)[a, b, axis] == g and hostio.elastic_lattice(key, 0.75, 4)[a, b, axis] == np.float32(0.75) * g
    assert np.array_equal(hostio.elastic_lattice(key, 1.0, 3), hostio.elastic_lattice(key, 1.0, 16)[:6, :6])   # the grid only cuts the lattice
    assert not np.array_equal(hostio.elastic_lattice(key, 1.0, 3), hostio.elastic_lattice(key + 1, 1.0, 3))


def test_elastic_draw_and_its_generator():
    a = np.random.RandomState(7)
    keys = pool.elastic_draw(a, 9, 4.0, 3)
    assert keys.dtype == np.uint32 and keys.shape == (9,)
    b = np.random.RandomState(7)
    assert keys.tolist() == [b.randint(0, 2 ** 32) for _ in range(9)]                       # one randint per sample, in order
    assert np.array_equal(keys, pool.elastic_draw(np.random.RandomState(7), 9, 4.0, 3))     # the same seed repeats the keys
    assert not np.array_equal(keys, pool.elastic_draw(np.random.RandomState(8), 9, 4.0, 3))
    assert len(set((keys >> 16).tolist())) > 6                                              # 32-bit keys, not small integers
    c = np.random.RandomState(7)
    assert not pool.elastic_draw(c, 5, 0.0, 3).any() and c.random_sample() == np.random.RandomState(7).random_sample()   # alpha 0: nothing drawn
    # the elastic generator is its own: affine_draw's stream stays where it was
    g1, g2, e = np.random.RandomState(11), np.random.RandomState(11), np.random.RandomState((11 + 0xbb67ae85) % 2 ** 32)
    kw = dict(rotation=30.0, scale=(0.8, 1.25), d4=True)
    m1 = pool.affine_draw(g1, 4, **kw)
    pool.elastic_draw(e, 4, 4.0, 3)
    m1b = pool.affine_draw(g1, 4, **kw)
    assert np.array_equal(m1, pool.affine_draw(g2, 4, **kw)) and np.array_equal(m1b, pool.affine_draw(g2, 4, **kw))
    assert pool.check_elastic((4, 3)) == (4.0, 3) and pool.check_elastic((0.0, 16)) == (0.0, 16)
    nan, inf = float("nan"), float("inf")
    for bad in ((1.0, 0), (1.0, 17), (-1.0, 3), (64.5, 3), (nan, 3), (inf, 3), (1.0, 3.0), (True, 3), (1.0, True), (1.0,), (1.0, 2, 3), None, 2.0, "x"):
        with pytest.raises(ValueError):
            pool.check_elastic(bad)
    with pytest.raises(ValueError):
        pool.elastic_draw(np.random.RandomState(0), 1, -1.0, 3)


def test_elastic_flag_and_command_line():
    assert len(FLAG_DEFS) == 30                                            # the reference's flags stay the reference's
    defs = {d[0]: d for d in EXTRA_FLAG_DEFS}
    assert defs["elastic_deformation"][1:3] == (str, "0,3")
    assert Options().elastic_deformation == (0.0, 3)
    o = parse_options(["--elastic_deformation=10,3", "--random_rotation=180", "--d4_augmentation"])
    assert o.elastic_deformation == (10.0, 3) and isinstance(o.elastic_deformation[1], int) and o.random_rotation == 180.0
    assert parse_options(["--elastic_deformation", "0.5,16"]).elastic_deformation == (0.5, 16)
    assert parse_options(["--elastic_deformation=64,1"]).elastic_deformation == (64.0, 1)
    assert Options(elastic_deformation=(2, 4)).elastic_deformation == (2.0, 4) and parse_elastic_deformation("0, 5") == (0.0, 5)
    nan = float("nan")
    for bad in ("1", "1,2,3", "", "nan,3", "inf,3", "-1,3", "64.5,3", "1,0", "1,17", "1,-2", "1,3.5", "1,3.0", "a,b", "1,", None, 1.0,
                (1.0, 3.0), (nan, 3), (True, 3), (1.0, True), (1.0,)):
        with pytest.raises(ValueError):
            Options(elastic_deformation=bad)
    for argv in (["--elastic_deformation=10"], ["--elastic_deformation=10,3,1"], ["--elastic_deformation=nan,3"], ["--elastic_deformation=-1,3"],
                 ["--elastic_deformation=65,3"], ["--elastic_deformation=1,0"], ["--elastic_deformation=1,17"], ["--elastic_deformation=1,2.5"]):
        with pytest.raises(ValueError):
            parse_options(argv)
    # with the host pool the flag is refused, not ignored
    with pytest.raises(ValueError, match="nodevice_patch_pool"):
        parse_options(["--elastic_deformation=2,3", "--nodevice_patch_pool"])
    assert parse_options(["--nodevice_patch_pool", "--elastic_deformation=0,5"]).device_patch_pool is False   # (alpha 0 is off)


def test_mirror_refuses_what_the_abi_refuses():
    ext, lab = au.make_images(2, 20, 4)
    I = np.eye(2)
    good = au.rec(0, 9.5, 9.5, I) + (2.0, 123, 3)
    x, y = hostio.elastic_patches(ext, lab, [good], 12, 4)
    assert x.shape == (1, 12, 12, 3) and y.shape == (1, 4, 4)
    nan, inf = float("nan"), float("inf")
    tail = (2.0, 123, 3)
    bads = [[au.rec(2, 9.5, 9.5, I) + tail], [au.rec(-1, 9.5, 9.5, I) + tail], [au.rec(0, nan, 9.5, I) + tail], [au.rec(0, 9.5, 9.5, 65.0 * I) + tail],
            [au.rec(0, 9.5, 9.5, [[1, inf], [0, 1]]) + tail], [au.rec(0, 9.5, 5.0e6, I) + tail], []]
    bads += [[good, au.rec(0, 9.5, 9.5, I) + (a, 1, 3)] for a in (nan, inf, -inf, -1.0, 64.5)]
    bads += [[good, au.rec(0, 9.5, 9.5, I) + (2.0, 1, g)] for g in (0, 17, -1)]
    for bad in bads:
        with pytest.raises(ValueError):
            hostio.elastic_patches(ext, lab, bad, 12, 4)
    for S, P in ((12, 5), (4, 12), (10, 4), (14, 4), (12, 0)):
        with pytest.raises(ValueError):
            hostio.elastic_patches(ext, lab, [good], S, P)
    with pytest.raises(ValueError):
        hostio.elastic_patches(ext.astype(np.float64), lab, [good], 12, 4)
    with pytest.raises(ValueError):
        hostio.elastic_patches(ext, lab[:1], [good], 12, 4)
    for bad_lat, S in ((np.zeros((3, 3, 2), np.float32), 12), (np.zeros((20, 20, 2), np.float32), 12), (np.zeros((6, 5, 2), np.float32), 12),
                       (np.zeros((6, 6, 3), np.float32), 12), (np.zeros((6, 6, 2), np.float32), 0)):
        with pytest.raises(ValueError):
            hostio.elastic_field(bad_lat, S)
    assert hostio.elastic_patches(ext, lab, [au.rec(0, 9.5, 9.5, I) + (64.0, 2 ** 32 - 1, 16), au.rec(1, 9.5, 9.5, I) + (0.0, 0, 1)], 12, 4)[0].shape[0] == 2


def test_abi_refuses_bad_arguments_on_the_host():
    """every refused call returns from host code before anything is launched (no GPU is needed: the device pointers are never
    dereferenced)"""
    from road_segmentation_unet_amd import _lib
    L = _lib.lib()
    assert ctypes.sizeof(_lib.RsuElastic) == hostio.ELASTIC_DTYPE.itemsize == 48 and _lib.ELASTIC_MAX_LAUNCH == 32 and _lib.ELASTIC_MAX_GRID == 16
    assert [n for n, _ in _lib.RsuElastic._fields_] == list(hostio.ELASTIC_DTYPE.names)
    assert [getattr(_lib.RsuElastic, n).offset for n, _ in _lib.RsuElastic._fields_] == [hostio.ELASTIC_DTYPE.fields[n][1] for n in hostio.ELASTIC_DTYPE.names]
    p = ctypes.c_void_p(4096)
    ok = dict(images=p, labels=p, x_out=p, labels_out=p, recs=[au.rec(0, 9.5, 9.5, np.eye(2)) + (2.0, 5, 3)], nimg=3, He=28, Hl=20, S=12, P=4)
    cases = eu.abi_cases()
    assert len(cases) == len(au.abi_cases()) + 10
    for name, b in cases:
        assert eu.abi_call(L, dict(ok, **b)) == -22, name
    assert eu.abi_call(L, dict(ok, He=13400 + 8, Hl=13400, S=12, P=4)) == _lib.E2BIG      # one image of 2.15 GB
