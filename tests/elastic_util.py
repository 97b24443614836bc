"""Shared by tests/test_elastic_host.py and tests/test_gpu_elastic.py: the geometries, the bank of elastic records (the one-launch loader's
bank crossed with grids, amplitudes and keys), the float64 restatement of the displacement field (include/rsu.h rsu_elastic_patches) with
its derived error bound, and the ABI's refused calls."""
import ctypes
import functools

import numpy as np

from road_segmentation_unet_amd import hostio
from tests import affine_util as au

# (Hl, offset, S, P): the loader's two, and one whose 400 window pixels make two workgroups per sample, the second one ragged (144 of 256
# lanes): the lanes past the last pixel sit behind the kernel's barrier
GEOMS = au.GEOMS + [(28, 4, 20, 12)]
STRIDE = {**au.STRIDE, 20: 4}
GRIDS = (1, 3, 16)              # 16: cells smaller than a pixel at S = 12
ALPHAS = (0.0, 0.75, 4.0)
NIMG = 3
MAX_G = 3.47                    # rsu.h: |g| <= 131070 C < 3.4641, so |u| <= 3.47 alpha


def affine_case(Hl, offset, S, P):
    """(ext, lab, recs, hx, hy) of tests/test_gpu_affine.py _case: the one-launch loader's images, its bank of 51 records and the host
    mirror's outputs for them"""
    from tests.test_gpu_affine import _case
    return _case(Hl, offset, S, P)


def elastic_of(affine_recs, alpha, key, grid):
    """ELASTIC_DTYPE records with the seven fields of `affine_recs` (AFFINE_DTYPE) and the given alpha, key, grid (scalars or arrays)"""
    recs = np.zeros(len(affine_recs), dtype=hostio.ELASTIC_DTYPE)
    for name in ("image", "cy", "cx", "m00", "m01", "m10", "m11"):
        recs[name] = affine_recs[name]
    recs["alpha"], recs["key"], recs["grid"] = alpha, key, grid
    return recs


@functools.lru_cache(maxsize=None)
def case(Hl, offset, S, P):
    """per geometry, computed once and left unchanged: the loader's images, the bank -- every record of the loader's bank under every
    (grid, alpha) of GRIDS x ALPHAS, record-major, each with a 32-bit key of its own (459 records) -- and the host mirror's outputs"""
    ext, lab, arecs, _, _ = affine_case(Hl, offset, S, P)
    combos = [(g, a) for g in GRIDS for a in ALPHAS]
    base = np.repeat(arecs, len(combos))
    grid = np.tile(np.array([g for g, _ in combos], np.int32), len(arecs))
    alpha = np.tile(np.array([a for _, a in combos], np.float32), len(arecs))
    keys = np.random.RandomState(23).randint(0, 2 ** 32, size=len(base)).astype(np.uint32)
    recs = elastic_of(base, alpha, keys, grid)
    hx, hy = hostio.elastic_patches(ext, lab, recs, S, P)
    hx.setflags(write=False), hy.setflags(write=False), recs.setflags(write=False)
    return ext, lab, recs, hx, hy


def field64(lattice, S):
    """float64 restatement of the field: the uniform cubic B-spline over the float32 lattice (taken as data) at t = (iw + 0.5) G / S per
    axis, with the textbook weights; [2][S][S]"""
    lat = np.asarray(lattice, dtype=np.float64)
    G = lat.shape[0] - 3
    t = (np.arange(S, dtype=np.float64) + 0.5) * G / S
    k = np.clip(np.floor(t).astype(np.int64), 0, G - 1)
    f = t - k
    w = np.stack([(1 - f) ** 3, 3 * f ** 3 - 6 * f ** 2 + 4, -3 * f ** 3 + 3 * f ** 2 + 3 * f + 1, f ** 3]) / 6.0
    u = np.zeros((2, S, S))
    for a in range(4):
        for b in range(4):
            u += (w[a][:, None] * w[b][None, :])[None] * np.moveaxis(lat[(k + a)[:, None], (k + b)[None, :]], -1, 0)
    return u


def weight_bound():
    """|float32 weight - exact weight| for one cubic B-spline weight at a given float32 fraction f in [0, 1], in absolute terms, derived:
    with e = 2^-24 (half an ulp of a value below 1), f2 = f * f carries e, f3 = f2 * f carries 2 e, g1 = 1 - f carries e. The widest
    bracket is w[1]'s: 3 f3 carries 3 * 2 e plus a rounding below 4 (2 e) = 8 e; 6 f2 carries 6 e plus a rounding below 8 (4 e) = 10 e; their
    difference adds a rounding below 4 (2 e): 20 e; + 4 adds a rounding below 4 (2 e): 22 e. (w[2]'s bracket carries 20 e by the same count,
    w[0]'s g1^3 carries 3 e + 2 e, w[3]'s f3 2 e.) Times SIXTH: 22 e / 6 < 3.7 e, plus SIXTH's own rounding (e / 2 relative, on a weight of
    at most 2 / 3) and the product's rounding (below 1: e) -- under 5 e in all."""
    return 5.0 * 2.0 ** -24


def field_bound(alpha, G, cmax=None):
    """|hostio.elastic_field - field64| at any pixel, derived, not tuned, from the count of roundings and the lattice's bound
    C = 3.47 alpha (or `cmax`, a bound of the lattice given). With e = 2^-24:
      coordinates  t = ((float)iw + 0.5f) * q: iw + 0.5 is exact, q = (float)(G / S) and the product round once each, so |dt| <= 2 e t
                   <= 2 e G. k and f = t - (float)k are then exact for the float32 t (a difference of neighbours on t's own grid), so
                   the float32 field is the spline evaluated AT the float32 t, which is continuous in t whatever cell k it falls in. The
                   spline's derivative along an axis is a convex combination of differences of neighbouring control points, at most 2 C:
                   2 C * 2 e G per axis, 8 G e C for both.
      weights      each within weight_bound() = 5 e of its exact value; the four exact weights of an axis are non-negative and sum to 1.
      a row        sum_b wx[b] c: the four weight errors move it by 4 * 5 e C, the four products round by e of |wx c| each (e C in
                   all), the three sums by e of a partial sum of at most C each: 24 e C.
      the field    sum_a wy[a] row_a: the rows' errors pass through with total weight 1 (24 e C), the four weight errors add 20 e C,
                   four products and three sums 4 e C more: 48 e C, rounded up to 50.
    Total: (50 + 8 G) e C."""
    C = MAX_G * float(alpha) if cmax is None else float(cmax)
    return (50.0 + 8.0 * G) * 2.0 ** -24 * C


def abi_cases():
    """(name, overrides of a good call) for every RSU_EINVAL case of rsu.h rsu_elastic_patches: everything rsu_affine_patches refuses (its
    records completed with a good alpha, key and grid), then the elastic fields' own cases"""
    nan, inf = float("nan"), float("inf")
    good = (2.0, 12345, 3)
    cases = []
    for name, b in au.abi_cases():
        if "recs" in b:
            b = dict(b, recs=[tuple(r) + good for r in b["recs"]])
        cases.append((name, b))
    base = au.rec(0, 9.5, 9.5, np.eye(2))
    for what, tail in [("alpha %r" % a, (a, 1, 3)) for a in (nan, inf, -inf, -1.0, -1e-30, 64.5)] \
            + [("grid %d" % g, (2.0, 1, g)) for g in (0, 17, -1, 1 << 20)]:
        cases.append((what, dict(recs=[base + good, base + tail])))
    return cases


def abi_call(L, a):
    from road_segmentation_unet_amd import _lib
    recs = hostio.elastic_records(a["recs"])
    rp = recs.ctypes.data_as(ctypes.c_void_p) if a.get("recs_ptr", 1) is not None else None
    nrec = a["nrec"] if "nrec" in a else len(recs)
    return L.rsu_elastic_patches(a["images"], a["labels"], ctypes.cast(rp, ctypes.POINTER(_lib.RsuElastic)), nrec, a["nimg"], a["He"], a["Hl"],
                                 a["S"], a["P"], a["x_out"], a["labels_out"], a.get("stream"))
