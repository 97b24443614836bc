"""Shared by tests/test_jitter_host.py and tests/test_gpu_jitter.py: the float64 sequential definition of the colour jitter (include/rsu.h
rsu_color_jitter; pool.jitter_draw) with its derived error bound, record builders, the mixed batches of the GPU tests and the ABI's refused
calls."""
import ctypes
import math

import numpy as np

from road_segmentation_unet_amd import _lib, hostio, pool

LUMA = np.array([0.299, 0.587, 0.114])
STRONG = (0.9, 0.9, 0.9, 180.0)            # large strengths: factors in [0.1, 1.9], any hue


def draw_params(rng, count, B, C, S, H):
    """(b, c, s, theta) per sample, restated from the order pool.jitter_draw documents (all four strengths above zero, no noise)"""
    out = []
    for _ in range(count):
        u = rng.random_sample(4)
        out.append((1.0 + (2.0 * u[0] - 1.0) * B, 1.0 + (2.0 * u[1] - 1.0) * C, 1.0 + (2.0 * u[2] - 1.0) * S, (2.0 * u[3] - 1.0) * H))
    return out


def sequential64(x, b, c, s, theta, clamp=True):
    """One sample [S][S][3] in float64, step by step: brightness, contrast about the per-channel mean of the brightened sample
    (tf.image.adjust_contrast), saturation towards luma, a rotation of the colour vector by theta degrees about the grey axis (Rodrigues'
    formula on the vectors, no matrix), then the clamp."""
    v = np.asarray(x, dtype=np.float64) * b
    m = v.mean(axis=(0, 1))
    v = (v - m) * c + m
    luma = (v * LUMA).sum(axis=-1, keepdims=True)
    v = luma + s * (v - luma)
    t = math.radians(theta)
    u = np.ones(3) / math.sqrt(3.0)
    v = v * math.cos(t) + np.cross(np.broadcast_to(u, v.shape), v) * math.sin(t) + u * (v @ u)[..., None] * (1.0 - math.cos(t))
    return np.clip(v, 0.0, 1.0) if clamp else v


def value_bound(recs):
    """|hostio.color_jitter - float64 definition| for data and means in [0, 1], derived, not tuned. Output row r is
    ((a0 x0 + a1 x1) + a2 x2) + ((k0 m0 + k1 m1) + k2 m2). With |x|, |m| <= 1 every intermediate is at most W = sum|a| + sum|k| of the row,
    and a float32 rounding of a value of magnitude v costs at most 2^-24 v. The longest chain of roundings behind an output is the means'
    path: the coefficient k (A and K are float64 matrices rounded once), the mean's conversion to float32, the product, the two sums of
    d_r, the final sum: 6 (the pixel's path has 5: coefficient, product, two sums, the final sum). Each costs at most 2^-24 W in total over
    the terms it touches. The mean itself is a sum of values quantised to 2^-24 steps (an error of at most 2^-25 each, so at most 2^-25 in
    the mean), weighted by the row's sum|k|. The clamp is 1-Lipschitz. (1 + 2^-20) covers the second-order terms."""
    recs = hostio.jitter_records(recs)
    sa = np.abs(recs["a"].astype(np.float64)).reshape(-1, 3, 3).sum(axis=2)
    sk = np.abs(recs["k"].astype(np.float64)).reshape(-1, 3, 3).sum(axis=2)
    return float((6.0 * 2.0 ** -24 * (sa + sk) + 2.0 ** -25 * sk).max()) * (1.0 + 2.0 ** -20)


def record(A=None, K=None, sigma=0.0, key=0):
    return (np.eye(3) if A is None else A, np.zeros((3, 3)) if K is None else K, sigma, key)


def identity(count=1):
    """`count` identity records: A = I, K = 0, sigma = 0"""
    return hostio.jitter_records([record()] * count)


def mixed_records(count, seed):
    """`count` records cycling through the four kinds, so that a sample that skips the means sits beside one that needs them: identity,
    contrast only (A = c I, K = (1 - c) I), noise only, all on (a strong draw with noise)"""
    rng = np.random.RandomState(seed)
    out = []
    for j in range(count):
        kind = j % 4
        if kind == 0:
            out.append(record())
        elif kind == 1:
            c = 0.25 + 1.5 * rng.random_sample()
            out.append(record(c * np.eye(3), (1.0 - c) * np.eye(3)))
        elif kind == 2:
            out.append(record(sigma=0.05 + 0.2 * rng.random_sample(), key=int(rng.randint(0, 2 ** 32))))
        else:
            (b, c, s, th), = draw_params(rng, 1, *STRONG)
            A, K = pool.jitter_matrices(b, c, s, th)
            out.append(record(A, K, 0.1 * rng.random_sample() + 0.01, int(rng.randint(0, 2 ** 32))))
    return hostio.jitter_records(out)


def make_batch(n, S, seed):
    """float32 [n][S][S][3] in [0, 1], each sample with a level of its own, and exact zeros and ones among the values"""
    rng = np.random.RandomState(seed)
    x = rng.rand(n, S, S, 3) * rng.uniform(0.3, 1.0, (n, 1, 1, 3))
    x[rng.rand(n, S, S, 3) < 0.02] = 0.0
    x[rng.rand(n, S, S, 3) < 0.02] = 1.0
    return x.astype(np.float32)


def abi_cases():
    """(name, overrides of a good call) for every RSU_EINVAL case of rsu.h rsu_color_jitter; `recs` overrides are lists of records"""
    nan, inf = float("nan"), float("inf")
    I, Z = np.eye(3), np.zeros((3, 3))
    cases = [("x", dict(x=None)), ("recs", dict(recs_ptr=None)), ("nrec 0", dict(nrec=0)), ("nrec -1", dict(nrec=-1)), ("S 0", dict(S=0)),
             ("S -1", dict(S=-1))]
    for i in (0, 4, 8):
        for v in (nan, inf, -inf, 64.5, -65.0):
            A, K = I.copy().reshape(9), Z.copy().reshape(9)
            A[i] = v
            cases.append(("a[%d] %r" % (i, v), dict(recs=[record(), record(A)])))
            K[i] = v
            cases.append(("k[%d] %r" % (i, v), dict(recs=[record(), record(I, K)])))
    cases += [("sigma %r" % v, dict(recs=[record(), record(sigma=v)])) for v in (nan, inf, -inf, -0.25, 1.5)]
    cases += [("NULL ws with a non-zero k", dict(ws=None, recs=[record(), record(I, 0.5 * I)])), ("ws misaligned", dict(ws_addr_add=4))]
    return cases


def abi_call(L, a):
    recs = hostio.jitter_records(a["recs"])
    rp = recs.ctypes.data_as(ctypes.c_void_p) if a.get("recs_ptr", 1) is not None else None
    nrec = a["nrec"] if "nrec" in a else len(recs)
    ws = a["ws"]
    if a.get("ws_addr_add"):
        ws = ctypes.c_void_p(ws.value + a["ws_addr_add"])
    return L.rsu_color_jitter(a["x"], ctypes.cast(rp, ctypes.POINTER(_lib.RsuJitter)), nrec, a["S"], ws, a.get("stream"))
