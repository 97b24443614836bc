"""Helpers for the -m gpu parity tests: move numpy data to the device as bf16/f32, call the C ABI, compare."""
import ctypes
import os

import numpy as np
import torch

from oracle import unet_oracle as U
from road_segmentation_unet_amd._lib import RsuSrc, call, lib

DEV = "cuda:0"
BF16_ULP = 2.0 ** -7  # worst-case relative spacing of bfloat16


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev_bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).to(torch.bfloat16).contiguous()


def dev_f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV).contiguous()


def host(t):
    torch.cuda.synchronize()
    return t.detach().to(torch.float32).cpu().numpy()


def ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def q(a):
    """bf16 round trip on the host (same RNE as the device)"""
    return U.round_bf16(np.asarray(a, dtype=np.float32))


def src_of(t, h, w, oy=None, ox=None):
    H, W, C = t.shape[1], t.shape[2], t.shape[3]
    return RsuSrc(t.data_ptr(), H, W, C, (H - h) // 2 if oy is None else oy, (W - w) // 2 if ox is None else ox)


def pack_conv_fwd(w, segs=None):
    k, cin, cout = w.shape[0], w.shape[2], w.shape[3]
    segs = segs or [cin]
    seg = (ctypes.c_int * len(segs))(*segs)
    nbytes = lib().rsu_packed_bytes(k * k, cout, seg, len(segs))
    out = torch.zeros(nbytes // 2, dtype=torch.bfloat16, device=DEV)
    wd = dev_f32(w)
    call("rsu_pack_conv_fwd", ptr(wd), ptr(out), k, cin, cout, seg, len(segs), stream())
    return out


def pack_conv_bwd(w, ci_off=0, ci_cnt=None):
    k, cin, cout = w.shape[0], w.shape[2], w.shape[3]
    ci_cnt = ci_cnt or cin
    seg = (ctypes.c_int * 1)(cout)
    out = torch.zeros(lib().rsu_packed_bytes(k * k, ci_cnt, seg, 1) // 2, dtype=torch.bfloat16, device=DEV)
    wd = dev_f32(w)
    call("rsu_pack_conv_bwd", ptr(wd), ptr(out), k, cin, ci_off, ci_cnt, cout, stream())
    return out


def assert_bf16_close(got, ref, what, ulps=1.0, atol_scale=2e-5):
    """got: device result that was rounded to bf16 once; ref: oracle result (float32, same bf16-rounded inputs).
    Allowed: `ulps` bf16 ulp of relative error (rounding-boundary flips from a different fp32 summation order)
    plus atol_scale * max|ref| (fp32 accumulation noise where the result cancels)."""
    got = np.asarray(got, np.float32)
    refq = q(ref)
    assert got.shape == refq.shape, (what, got.shape, refq.shape)
    scale = float(np.abs(refq).max()) if refq.size else 1.0
    tol = ulps * BF16_ULP * np.abs(refq) + atol_scale * max(scale, 1e-30)
    err = np.abs(got - refq)
    bad = ~(err <= tol)   # (a NaN left in the output is out of tolerance too: NaN > tol is False)
    if bad.any():
        idx = np.unravel_index(np.argmax(np.where(np.isnan(err), np.inf, err - tol)), err.shape)
        raise AssertionError("%s: %d/%d elements out of tolerance; worst at %s got %r ref %r (max|ref| %g); exact-match frac %.4f"
                             % (what, int(bad.sum()), bad.size, idx, got[idx], refq[idx], scale, float((got == refq).mean())))
    return float((got == refq).mean())


ROUNDED_MAX_MISMATCH = 0.01   # share of counted elements whose bits differ from q(ref)
ROUNDED_MAX_BIAS = 0.02       # |mean signed error| in ulps
ROUNDED_MIN_COUNT = 10000     # counted elements
ROUNDED_MIN_SHARE = 0.35      # counted / all


def assert_bf16_rounded(got, ref, what):
    """got: device result that was rounded to bf16 ONCE, to nearest, from an fp32 accumulator; ref: the oracle's float result (or a float64
    array) on the same bf16-rounded inputs, NOT rounded. First assert_bf16_close(got, ref, what), unchanged. Then, over the counted
    elements (q(ref) finite and non-zero), with ulp = 2^(floor(log2 |q(ref)|) - 7):
      mismatch = mean(got != q(ref)) <= 0.01. A correct kernel flips only where fp32 summation noise straddles a rounding boundary
                 (about 1e-4); a truncating store gives 0.5, a second rounding 0.3 or more: a factor 100 below, 30 above.
      bias     = |mean(sign(ref) (got - ref) / ulp)| <= 0.02. Round-to-nearest gives 0 with standard error 0.29 / sqrt(n), at most 0.003
                 at n = 10,000; truncation gives -0.5.
    Conditions (asserted, so that no case passes on a handful of elements): at least 10,000 counted elements and at least 35 % of the
    output counted. Returns (mismatch, bias, n). With RSU_ROUNDING_RECORD=<file> set, appends the three figures to that file."""
    assert_bf16_close(got, ref, what)
    got = np.asarray(got, np.float32)
    ref64 = np.asarray(ref, np.float64)
    refq = q(ref)
    counted = np.isfinite(refq) & (refq != 0)
    n = int(counted.sum())
    share = n / max(1, refq.size)
    if n < ROUNDED_MIN_COUNT or share < ROUNDED_MIN_SHARE:
        raise AssertionError("%s: rounding statistic not measurable: %d counted elements (at least %d), share %.3f of %d (at least %.2f)"
                             % (what, n, ROUNDED_MIN_COUNT, share, refq.size, ROUNDED_MIN_SHARE))
    g, r, rq = got[counted].astype(np.float64), ref64[counted], refq[counted].astype(np.float64)
    ulp = 2.0 ** (np.floor(np.log2(np.abs(rq))) - 7)
    mismatch = float((g != rq).mean())
    bias = float((np.sign(r) * (g - r) / ulp).mean())
    rec = os.environ.get("RSU_ROUNDING_RECORD")
    if rec:
        with open(rec, "a") as f:
            f.write("%-72s mismatch %.6f  bias %+.5f  n %d\n" % (what, mismatch, bias, n))
    if mismatch > ROUNDED_MAX_MISMATCH or abs(bias) > ROUNDED_MAX_BIAS:
        d = np.abs(g - rq) / ulp
        k = int(np.argmax(d))
        idx = tuple(int(a[k]) for a in np.nonzero(counted))
        raise AssertionError("%s: not one round-to-nearest of an fp32 sum: mismatch %.4f (limit %.2f), bias %+.4f ulp (limit %.2f), n %d; "
                             "worst at %s got %r q(ref) %r ref %r (%.2f ulp)"
                             % (what, mismatch, ROUNDED_MAX_MISMATCH, bias, ROUNDED_MAX_BIAS, n, idx, float(g[k]), float(rq[k]), float(r[k]), float(d[k])))
    return mismatch, bias, n


def assert_f32_close(got, ref, what, rtol=1e-4, atol_scale=1e-5):
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    scale = float(np.abs(ref).max()) if ref.size else 1.0
    tol = rtol * np.abs(ref) + atol_scale * max(scale, 1e-30)
    err = np.abs(got - ref)
    bad = ~(err <= tol)   # (NaN included)
    if bad.any():
        idx = np.unravel_index(np.argmax(np.where(np.isnan(err), np.inf, err - tol)), err.shape)
        raise AssertionError("%s: %d/%d out of tolerance; worst at %s got %r ref %r (max|ref| %g)"
                             % (what, int(bad.sum()), err.size, idx, got[idx], ref[idx], scale))
