"""Helpers for the tests at the 2-GiB tensor limit (tests/test_gpu_large_tensors.py, tests/test_large_limits_host.py).

A tensor just under 2 GiB cannot go through the CPU oracle, and does not have to: every batch kernel treats images independently. The
batch is PERIODIC, x[n] = base[n % K] with K seeded, bf16-rounded images built on the device; the reference is the oracle on those K
images, uploaded once; the comparison runs on the device in chunks of at most 256 MiB of output with the tolerance rule of
hiputil.assert_bf16_close / assert_f32_close restated in torch (same constants, imported). No whole tensor ever comes to the host."""
import numpy as np
import pytest
import torch

from oracle import unet_oracle as U
from tests import hiputil as hu

LIMIT = 0x7ffffff0          # a tensor of LIMIT bytes or more is refused (RSU_E2BIG): rsu_api.hip, UNet._check_tensor_sizes
K = 3                       # distinct images of a periodic batch
CHUNK_BYTES = 256 << 20     # of the tensor under comparison, per step
MIN_FREE_BYTES = 32 << 30   # below this much free device memory a large test may skip (an MI355X has 288 GB)
# the tolerance constants are hiputil's own, read from its two functions' defaults (2^-7 is hu.BF16_ULP): nothing is restated here
BF16_ULPS, BF16_ATOL_SCALE = hu.assert_bf16_close.__defaults__
F32_RTOL, F32_ATOL_SCALE = hu.assert_f32_close.__defaults__

RECORD = []   # one dict per comparison: what, N, bytes, worst error -- a job script may dump it (profiles/r22/large_tensors.txt)


def note(what, N, nbytes, got, ref):
    """record a small host-side comparison (a weight gradient, a sum): worst |got - ref| beside max|ref|"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    RECORD.append(dict(what=what, N=int(N), bytes=int(nbytes), worst_err=float(np.abs(got - ref).max()), scale=float(np.abs(ref).max())))


def n_max(bytes_per_image):
    """the largest N with N * bytes_per_image < LIMIT"""
    return (LIMIT - 1) // int(bytes_per_image)


def straddler(bytes_per_image):
    """the image that holds byte 2^30 of a tensor"""
    return (1 << 30) // int(bytes_per_image)


def need_memory():
    free, _ = torch.cuda.mem_get_info()
    if free < MIN_FREE_BYTES:
        pytest.skip("not enough free device memory: %.1f GiB free, the tests at the 2-GiB limit want 32 GiB" % (free / 2.0 ** 30))
    torch.cuda.reset_peak_memory_stats()


def done(*tensors):
    """every test ends here: nothing of it stays on the device"""
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated()
    assert peak <= 24 << 30, "a large test may allocate 24 GiB at the most, this one reached %.1f" % (peak / 2.0 ** 30)
    for r in RECORD:
        r.setdefault("peak_gib", peak / 2.0 ** 30)
    del tensors
    torch.cuda.empty_cache()


def base_images(seed, shape, scale=1.0, relu=False):
    """K seeded, bf16-rounded images, float32 on the host: [K, *shape]"""
    a = (np.random.RandomState(seed).standard_normal((K,) + tuple(shape)) * scale).astype(np.float32)
    return hu.q(np.maximum(a, 0) if relu else a)


def periodic(base, N, dtype=torch.bfloat16):
    """device tensor [N, *base.shape[1:]] with x[n] = base[n % K]; base: host array [K, ...] (exact in `dtype`)"""
    b = torch.from_numpy(np.ascontiguousarray(base)).to(hu.DEV).to(dtype)
    assert b.shape[0] == K
    out = torch.empty((N,) + tuple(b.shape[1:]), dtype=dtype, device=hu.DEV)
    full = N // K
    if full:
        out[:full * K].view((full, K) + tuple(b.shape[1:])).copy_(b.unsqueeze(0).expand((full, K) + tuple(b.shape[1:])))
    if N - full * K:
        out[full * K:].copy_(b[:N - full * K])
    return out


def sparse(per_image, N, shape, dtype=torch.bfloat16):
    """device tensor [N, *shape] of zeros but for the images of `per_image`, a dict n -> host array (exact in `dtype`)"""
    out = torch.zeros((N,) + tuple(shape), dtype=dtype, device=hu.DEV)
    for n, a in per_image.items():
        out[n].copy_(torch.from_numpy(np.ascontiguousarray(a)).to(hu.DEV).to(dtype))
    return out


def nan_out(shape, dtype=torch.bfloat16):
    return torch.full(tuple(shape), float("nan"), dtype=dtype, device=hu.DEV)


def _chunks(out):
    """(first image, image count) steps over out [N, ...]: whole periods of at most CHUNK_BYTES, then the rest"""
    N = out.shape[0]
    per = out[0].numel() * out.element_size()
    m = max(K, CHUNK_BYTES // per // K * K)
    n0 = 0
    while n0 < N:
        c = min(m, N - n0)
        if c > K:
            c = c // K * K
        yield n0, c
        n0 += c


def _compare(out, ref, what, tol_of, cast):
    """out [N, ...] on the device against ref [K, ...] (device, float): every image, in chunks; raises with the worst image and byte"""
    N = out.shape[0]
    per = out[0].numel()
    worst, worst_at, nbad, peak_err = -float("inf"), None, 0, 0.0
    tol = tol_of(ref)
    for n0, c in _chunks(out):
        got = cast(out[n0:n0 + c])
        if c % K == 0:
            g = got.view((c // K, K) + tuple(ref.shape[1:]))
            err = (g - ref.unsqueeze(0)).abs_()
            t = tol.unsqueeze(0)
        else:   # the tail: fewer than K images, starting at a multiple of K
            assert n0 % K == 0 and c < K
            err = (got - ref[:c]).abs_()
            t = tol[:c]
        bad = ~(err <= t)   # (a NaN left in the output is out of tolerance too)
        nb = int(bad.sum().item())
        finite = torch.nan_to_num(err, nan=0.0, posinf=0.0)
        peak_err = max(peak_err, float(finite.max().item()))
        if nb:
            nbad += nb
            excess = torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err - t).reshape(-1)
            i = int(torch.argmax(excess).item())
            if float(excess[i].item()) > worst:
                worst = float(excess[i].item())
                n, e = n0 + i // per, i % per
                worst_at = (n, (n * per + e) * out.element_size(), float(got.reshape(-1)[i].item()), float(ref[n % K].reshape(-1)[e].item()))
        del got, err, bad, finite
    RECORD.append(dict(what=what, N=N, bytes=N * per * out.element_size(), worst_err=peak_err, scale=float(ref.abs().max().item())))
    if nbad:
        raise AssertionError("%s: %d/%d elements out of tolerance; worst in image %d of %d at byte offset %d (0x%x): got %r ref %r"
                             % (what, nbad, N * per, worst_at[0], N, worst_at[1], worst_at[1], worst_at[2], worst_at[3]))
    return peak_err


def assert_bf16_periodic(out, ref, what, ulps=BF16_ULPS):
    """hiputil.assert_bf16_close for every image of out (bf16 [N, ...]) against ref [K, ...] (host, the oracle's float result):
    |got - q(ref)| <= ulps * BF16_ULP |q(ref)| + atol_scale max|q(ref)|"""
    assert out.dtype == torch.bfloat16 and tuple(out.shape[1:]) == tuple(ref.shape[1:]) and ref.shape[0] == K, (what, out.shape, ref.shape)
    refq = torch.from_numpy(hu.q(ref)).to(hu.DEV)

    def tol_of(r):
        return ulps * hu.BF16_ULP * r.abs() + BF16_ATOL_SCALE * max(float(r.abs().max().item()), 1e-30)
    return _compare(out, refq, what, tol_of, lambda t: t.to(torch.float32))


def assert_f32_periodic(out, ref, what, rtol=F32_RTOL, atol_scale=F32_ATOL_SCALE):
    """hiputil.assert_f32_close for every image of out (f32 [N, ...]) against ref [K, ...] (host), in float64"""
    assert out.dtype == torch.float32 and tuple(out.shape[1:]) == tuple(ref.shape[1:]) and ref.shape[0] == K, (what, out.shape, ref.shape)
    r64 = torch.from_numpy(np.ascontiguousarray(ref, dtype=np.float64)).to(hu.DEV)

    def tol_of(r):
        return rtol * r.abs() + atol_scale * max(float(r.abs().max().item()), 1e-30)
    return _compare(out, r64, what, tol_of, lambda t: t.to(torch.float64))


def assert_periodic_bits(out, what):
    """the second, sharper assertion where a kernel's summation order does not depend on the tile: out[n] == out[n % K], bit for bit"""
    bits = out.view({1: torch.uint8, 2: torch.int16, 4: torch.int32}[out.element_size()])
    first = bits[:K]
    for n0, c in _chunks(bits):
        if c % K == 0:
            same = bits[n0:n0 + c].view((c // K, K) + tuple(first.shape[1:])) == first.unsqueeze(0)
        else:
            same = bits[n0:n0 + c] == first[:c]
        if not bool(same.all().item()):
            i = int(torch.argmin(same.reshape(-1).to(torch.uint8)).item())
            per = first[0].numel()
            raise AssertionError("%s: image %d differs from image %d at byte offset %d" % (what, n0 + i // per, (n0 + i // per) % K,
                                                                                         (n0 * per + i) * out.element_size()))


def assert_no_nan(out, what):
    for n0, c in _chunks(out):
        assert not bool(torch.isnan(out[n0:n0 + c]).any().item()), "%s: NaN left in images %d..%d" % (what, n0, n0 + c - 1)


def mask_range(start, count, keep, key):
    """U.dropout_mask for the elements [start, start + count) of a tensor (the oracle's function has no offset and would build the
    whole 2^30-element array): the same hash on the same counters. tests/test_large_limits_host.py holds it to U.dropout_mask."""
    assert 0 <= start and start + count <= 0xFFFFFFFF
    with np.errstate(over="ignore"):
        h = (np.arange(count, dtype=np.uint64) + np.uint64(start)).astype(np.uint32) ^ np.uint32(key)
        h ^= h >> np.uint32(16)
        h *= np.uint32(0x85EBCA6B)
        h ^= h >> np.uint32(13)
        h *= np.uint32(0xC2B2AE35)
        h ^= h >> np.uint32(16)
    u = (h >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return np.floor(np.float32(keep) + u).astype(np.float32)


# ---- the limit of every batch-taking entry point, as bytes per image of each tensor the entry is handed (include/rsu.h states the
# same per entry). An entry takes N images iff N * max(bytes) < LIMIT. tests/test_large_limits_host.py holds the C ABI and _lib.call to
# this table at n_max + 1 (refused before anything is launched); tests/test_gpu_large_tensors.py runs every entry at n_max.
def _conv(H, W, Cin, Cout, dil=1):
    return [H * W * Cin * 2, (H - 2 * dil) * (W - 2 * dil) * Cout * 2]


LIMITS = {
    "rsu_conv2d_fwd": lambda H, W, Cin, Cout, dil=1: _conv(H, W, Cin, Cout, dil),
    "rsu_conv2d_fwd_pool": lambda H, W, Cin, Cout: _conv(H, W, Cin, Cout),
    "rsu_conv2d_bwd_data": lambda H, W, Cin, Cout, dil=1: _conv(H, W, Cin, Cout, dil),           # dx [H][W][Cin], dz the conv's output
    "rsu_conv2d_bwd_weight": lambda H, W, Cin, Cout, dil=1: _conv(H, W, Cin, Cout, dil),
    "rsu_wgrad_group_plan": lambda H, W, Cin, Cout, dil=1: _conv(H, W, Cin, Cout, dil),
    "rsu_convT2x2_fwd": lambda H, W, Cin, Cout: [H * W * Cin * 2, 4 * H * W * Cout * 2],
    "rsu_convT2x2_bwd_data": lambda H, W, Cin, Cout: [H * W * Cin * 2, 4 * H * W * Cout * 2],
    "rsu_convT2x2_bwd_weight": lambda H, W, Cin, Cout: [H * W * Cin * 2, 4 * H * W * Cout * 2],
    "rsu_conv_first_fwd": lambda H, W, Cout, dil=1: [H * W * 32, (H - 2 * dil) * (W - 2 * dil) * Cout * 2],
    "rsu_color_conv_first_fwd": lambda H, W, Cout, dil=1: [H * W * 12, (H - 2 * dil) * (W - 2 * dil) * Cout * 2],
    "rsu_conv_first_bwd_weight": lambda H, W, Cout, dil=1: [H * W * 32, (H - 2 * dil) * (W - 2 * dil) * Cout * 2],
    "rsu_maxpool2x2_fwd_code": lambda H, W, C: [H * W * C * 2],
    "rsu_pool_skip_relu_bwd_code": lambda H, W, C: [H * W * C * 2],
    "rsu_pool_skip_relu_bwd": lambda H, W, C: [H * W * C * 2],
    "rsu_dropout_fwd": lambda H, W, C: [H * W * C * 2],
    "rsu_color_adjust_fwd": lambda H, W: [H * W * 32],
    "rsu_head_fwd_bwd": lambda H, W, C: [H * W * C * 2],
    "rsu_head_eval": lambda H, W, C: [H * W * C * 2],
    "rsu_bias_grad": lambda H, W, C: [H * W * C * 2],
}


def entry_n_max(name, *geo, **kw):
    return n_max(max(LIMITS[name](*geo, **kw)))
