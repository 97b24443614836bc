"""Shared by tests/test_affine_host.py and tests/test_gpu_affine.py: the test images, record builders, the float64 restatement of the
one-launch loader's rule (include/rsu.h rsu_affine_patches) with its derived error bound, and the ABI's refused calls."""
import ctypes
import itertools
import math

import numpy as np

from road_segmentation_unet_amd import hostio

D4_OPS = list(itertools.product((False, True), (False, True), (False, True), range(4)))   # every draw d4_draw can make: 32, 8 distinct results


def make_images(nimg=3, Hl=20, offset=4, seed=0):
    """(extended float32 [nimg][Hl + 2 offset]^2[3], labels uint8 [nimg][Hl][Hl]): positive, non-symmetric images extended by their own
    mirror (what the pool holds for an unrotated image), labels a thresholded channel with an asymmetric block"""
    rng = np.random.RandomState(seed)
    orig = (0.05 + rng.rand(nimg, Hl, Hl, 3)).astype(np.float32)
    orig += (np.arange(Hl, dtype=np.float32) / Hl)[None, :, None, None]          # a vertical ramp: no symmetry survives
    lab = (orig[..., 1] > 0.9).astype(np.uint8)
    lab[:, 2:7, 1:Hl // 2] = 1
    return hostio.mirror_border(orig, offset), lab


def rec(image, cy, cx, M):
    M = np.asarray(M, dtype=np.float32)
    return (image, cy, cx, M[0, 0], M[0, 1], M[1, 0], M[1, 1])


def bilinear64(ext, lab, recs, S, P):
    """float64 restatement: bilinear interpolation of the symmetric-padded ORIGINAL image (np.pad repeats the reflection as often as
    needed) at centre + M d; returns (x float64, label VALUES float64 before the 0.5 threshold)"""
    He, Hl = ext.shape[1], lab.shape[1]
    offset = (He - Hl) // 2
    recs = hostio.affine_records(recs)
    pad = 8 * Hl

    def sample(a, r, n):
        d = np.arange(n, dtype=np.float64) - (n - 1) / 2.0
        di, dj = d[:, None], d[None, :]
        sy = (float(r["cy"]) - offset) + (float(r["m00"]) * di + float(r["m01"]) * dj) + pad
        sx = (float(r["cx"]) - offset) + (float(r["m10"]) * di + float(r["m11"]) * dj) + pad
        y0, x0 = np.floor(sy).astype(np.int64), np.floor(sx).astype(np.int64)
        fy, fx = sy - y0, sx - x0
        if a.ndim == 3:
            fy, fx = fy[..., None], fx[..., None]
        return (a[y0, x0] * (1 - fx) + a[y0, x0 + 1] * fx) * (1 - fy) + (a[y0 + 1, x0] * (1 - fx) + a[y0 + 1, x0 + 1] * fx) * fy

    xs, ys = [], []
    for r in recs:
        n = int(r["image"])
        img = np.pad(ext[n, offset:offset + Hl, offset:offset + Hl].astype(np.float64), ((pad, pad), (pad, pad), (0, 0)), mode="symmetric")
        lb = np.pad(lab[n].astype(np.float64), pad, mode="symmetric")
        xs.append(sample(img, r, S))
        ys.append(sample(lb, r, P))
    return np.stack(xs), np.stack(ys)


GEOMS = [(20, 4, 12, 4), (20, 3, 11, 5)]   # (Hl, offset, S, P): a half-integer centre and an integer one
STRIDE = {12: 4, 11: 5}                    # by S: a stride that tiles the geometry


DYADIC = [0.5 * np.eye(2), np.array([[1.0, 0.25], [0.0, 1.0]])]


def value_bound(ext, lab, recs, S):
    """|float32 mirror - float64 restatement| for the image values, derived, not tuned. A coordinate s = (c - offset) + (a di + b dj) takes
    five float32 roundings (c - offset, two products, their sum, the final sum), each at most half an ulp of the largest magnitude C any
    of them can reach: |ds| <= 2.5 ulp(C) per axis. Bilinear interpolation of the symmetric-padded image is continuous and piecewise linear
    with slope at most G per axis, G the largest difference of two neighbouring pixels (crossing into the next cell included: the
    function is continuous there), so the two coordinates move the value by at most 2 * G * 2.5 ulp(C). The fractions are exact
    differences. The interpolation itself rounds nine times (six products, three sums) on values of at most V, 2^-24 V each at most, and
    the roundings of 1 - fx and 1 - fy (2^-25 each) weigh values of at most V: 10 * 2^-24 * V more."""
    He, Hl = ext.shape[1], lab.shape[1]
    offset = (He - Hl) // 2
    recs = hostio.affine_records(recs)
    orig = ext[:, offset:offset + Hl, offset:offset + Hl].astype(np.float64)
    G = max(float(np.abs(np.diff(orig, axis=1)).max()), float(np.abs(np.diff(orig, axis=2)).max()))
    V = float(orig.max())
    half = (S - 1) / 2.0
    C = max(max(abs(float(r["cy"]) - offset), abs(float(r["cx"]) - offset))
            + half * max(abs(float(r["m00"])) + abs(float(r["m01"])), abs(float(r["m10"])) + abs(float(r["m11"]))) for r in recs)
    return 5.0 * G * float(np.spacing(np.float32(C))) + 10.0 * 2.0 ** -24 * V


def rotation_records(rng, count, nimg, Hl, offset, zooms=(0.25, 3.0), spread=3.0):
    """seeded rotations with zooms from 0.25 (a window several images wide: more than one reflection period) to 3, centred anywhere up to
    `spread` image widths outside the image"""
    out = []
    for k in range(count):
        th = rng.uniform(-math.pi, math.pi)
        s = math.exp(rng.uniform(math.log(zooms[0]), math.log(zooms[1]))) if k else zooms[0]
        M = (1.0 / s) * np.array([[math.cos(th), -math.sin(th)], [math.sin(th), math.cos(th)]])
        cy, cx = offset + rng.uniform(-spread * Hl, (spread + 1) * Hl, 2) if k % 2 else offset + rng.uniform(0, Hl, 2)
        out.append(rec(k % nimg, np.float32(cy), np.float32(cx), M))
    return out


def abi_cases():
    """(name, overrides of a good call) for every RSU_EINVAL case of rsu.h rsu_affine_patches; `recs` overrides are lists of records"""
    I = np.eye(2)
    nan, inf = float("nan"), float("inf")
    cases = [(k, {k: None}) for k in ("images", "labels", "recs_ptr", "x_out", "labels_out")]
    cases += [("nrec 0", dict(nrec=0)), ("nrec -1", dict(nrec=-1)), ("nimg 0", dict(nimg=0)), ("S < P", dict(S=2, He=18)), ("P 0", dict(P=0, S=8)),
              ("Hl 0", dict(Hl=0, He=8)), ("odd differences", dict(He=27, S=11)), ("S - P odd", dict(S=11)), ("He - Hl odd", dict(He=27)),
              ("offsets differ", dict(He=26)), ("He < Hl", dict(He=12, S=-4)),
              ("image -1", dict(recs=[rec(-1, 9.5, 9.5, I)])), ("image nimg", dict(recs=[rec(0, 9.5, 9.5, I), rec(3, 9.5, 9.5, I)])),
              ("m > 64", dict(recs=[rec(0, 9.5, 9.5, [[1, 0], [0, 64.5]])])), ("m < -64", dict(recs=[rec(0, 9.5, 9.5, [[-65, 0], [0, 1]])])),
              ("centre too far", dict(recs=[rec(0, 9.5, 5.0e6, I)]))]
    for f in range(6):
        for v in (nan, inf, -inf):
            vals = [9.5, 9.5, 1.0, 0.0, 0.0, 1.0]
            vals[f] = v
            cases.append(("field %d %r" % (f, v), dict(recs=[rec(0, 9.5, 9.5, I), (1,) + tuple(vals)])))
    return cases


def abi_call(L, a):
    recs = hostio.affine_records(a["recs"])
    rp = recs.ctypes.data_as(ctypes.c_void_p) if a.get("recs_ptr", 1) is not None else None
    nrec = a["nrec"] if "nrec" in a else len(recs)
    from road_segmentation_unet_amd import _lib
    return L.rsu_affine_patches(a["images"], a["labels"], ctypes.cast(rp, ctypes.POINTER(_lib.RsuAffine)), nrec, a["nimg"], a["He"], a["Hl"],
                                a["S"], a["P"], a["x_out"], a["labels_out"], a.get("stream"))
