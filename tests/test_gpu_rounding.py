"""-m gpu: every bf16-writing path rounds ONCE, to nearest, from its fp32 accumulator (README / DESIGN "bf16 storage, fp32 accumulate, RNE").
The op tests allow one full bf16 ulp per element, which a truncating store, a second rounding or bf16 partial sums all fit into. Here
each path's output goes through hiputil.assert_bf16_rounded: against the oracle (double accumulate, one rounding) at most 1 % of the
counted elements may differ in their bits and the mean signed error may be at most 0.02 ulp -- limits derived in the helper's docstring,
proven to separate right from wrong on the CPU in tests/test_rounding_host.py. Every launch is one an op test already makes (the call is
copied from it, seeds included; only the batch N grows where 10,000 counted elements need it). Where the design itself rounds twice (the
pool's dropout, the accumulating backward-data, the 1/keep pass behind the transposed conv's backward-data) the reference restates exactly
those roundings and is held to the same limits. RSU_ROUNDING_RECORD=<file> makes the
helper append every case's (mismatch, bias, n): profiles/r16/rounding.txt."""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_oracle as U  # noqa: E402
from tests import hiputil as hu  # noqa: E402
from tests.head_util import LAM, NPIX, SMOOTH, Ref, _batch, _dev_labels, _inputs, _weight_map  # noqa: E402
from road_segmentation_unet_amd._lib import RsuSrc, call, lib  # noqa: E402


def _rand(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def _nan(*shape):
    return torch.full(shape, float("nan"), dtype=torch.bfloat16, device=hu.DEV)


def _plan_lines(capfd):
    return [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[plan fwd2]")]


# the forced tile shapes and kernel generations of test_gpu_cfg_matrix.forced_cfg
FORCED = [(c, g) for c in range(8) for g in (2, 4) if not (g == 4 and c >= 6)]
forced = pytest.mark.parametrize("cfg,gen", FORCED, ids=["cfg%d-gen%d" % cg for cg in FORCED])


def _force(monkeypatch, cfg, gen):
    monkeypatch.setenv("RSU_FWD2_CFG", str(cfg))
    monkeypatch.setenv("RSU_FWD_GEN", str(gen))


# ------------------------------------------------------------------------------------------- 3x3 forward
def _conv_fwd(x, w, b, dil, relu):
    N, H, W, _ = x.shape
    Cout = w.shape[3]
    xd, wp, bd = hu.dev_bf16(x), hu.pack_conv_fwd(w), hu.dev_f32(b)
    y = _nan(N, H - 2 * dil, W - 2 * dil, Cout)
    s = (RsuSrc * 1)(hu.src_of(xd, H, W))
    call("rsu_conv2d_fwd", s, 1, hu.ptr(wp), hu.ptr(bd), hu.ptr(y), N, H, W, Cout, dil, relu, 0, hu.stream())
    return hu.host(y)


@pytest.mark.parametrize("N,H,W,Cin,Cout,dil,relu", [(2, 37, 41, 64, 64, 1, 1), (2, 37, 41, 64, 64, 1, 0), (1, 40, 36, 96, 128, 2, 1),
                                                     (1, 40, 36, 96, 128, 2, 0)])
def test_conv2d_fwd_default_plan(N, H, W, Cin, Cout, dil, relu):
    """test_gpu_ops.test_conv2d_fwd's launch: the planner's own tile shape, and the dilation-2 kernel"""
    rng = np.random.RandomState(Cin * 7 + Cout + H)
    x = hu.q(_rand(rng, N, H, W, Cin))
    w = _rand(rng, 3, 3, Cin, Cout, scale=1.0 / np.sqrt(9 * Cin))
    b = _rand(rng, Cout, scale=0.1)
    ref = U.conv2d_fwd(x, hu.q(w), b, dil=dil, relu=bool(relu))
    hu.assert_bf16_rounded(_conv_fwd(x, w, b, dil, relu), ref, "conv2d_fwd %dx%dx%dx%d->%d dil %d relu %d" % (N, H, W, Cin, Cout, dil, relu))


@functools.lru_cache(maxsize=None)
def _cfg_case():
    """test_gpu_cfg_matrix.test_conv3x3_fwd_and_bwd_data_every_shape at (1, 70, 75, 64, 192): inputs and both references, computed once"""
    N, H, W, Cin, Cout = 1, 70, 75, 64, 192
    rng = np.random.RandomState(H + Cout)
    x = hu.q(_rand(rng, N, H, W, Cin))
    w = _rand(rng, 3, 3, Cin, Cout, scale=1.0 / np.sqrt(9 * Cin))
    b = _rand(rng, Cout, scale=0.1)
    dz = hu.q(_rand(rng, N, H - 2, W - 2, Cout, scale=0.1))
    ref_y = U.conv2d_fwd(x, hu.q(w), b)
    ref_dx = U.relu_bwd(x, U.conv2d_bwd_data(dz, hu.q(w), (H, W)))
    return x, w, b, dz, ref_y, ref_dx


@forced
def test_conv2d_fwd_every_forced_shape(cfg, gen, monkeypatch):
    x, w, b, dz, ref_y, _ = _cfg_case()
    _force(monkeypatch, cfg, gen)
    hu.assert_bf16_rounded(_conv_fwd(x, w, b, 1, 1), ref_y, "conv2d_fwd 1x70x75x64->192 RSU_FWD2_CFG=%d RSU_FWD_GEN=%d" % (cfg, gen))


def test_conv2d_fwd_three_cropped_sources():
    """test_gpu_ops.test_conv2d_fwd_three_cropped_sources"""
    rng = np.random.RandomState(5)
    N, h, w = 2, 22, 26
    a = hu.q(_rand(rng, N, 34, 38, 32))
    bsrc = hu.q(_rand(rng, N, 28, 30, 32))
    c = hu.q(_rand(rng, N, h, w, 32))
    W = _rand(rng, 3, 3, 96, 64, scale=0.05)
    bias = _rand(rng, 64, scale=0.1)
    ad, bd_, cd = hu.dev_bf16(a), hu.dev_bf16(bsrc), hu.dev_bf16(c)
    wp = hu.pack_conv_fwd(W, [32, 32, 32])
    y = _nan(N, h - 2, w - 2, 64)
    srcs = (RsuSrc * 3)(hu.src_of(ad, h, w), hu.src_of(bd_, h, w), hu.src_of(cd, h, w))
    biasd = hu.dev_f32(bias)
    call("rsu_conv2d_fwd", srcs, 3, hu.ptr(wp), hu.ptr(biasd), hu.ptr(y), N, h, w, 64, 1, 1, 0, hu.stream())
    cat = np.concatenate([U.center_crop(a, h, w), U.center_crop(bsrc, h, w), c], axis=3)
    hu.assert_bf16_rounded(hu.host(y), U.conv2d_fwd(cat, hu.q(W), bias, relu=True), "conv2d_fwd three cropped sources 32+32+32->64")


@pytest.mark.parametrize("N,H,W,segs,Cout", [(1, 20, 20, [512], 512), (1, 20, 20, [200, 120], 128)])
def test_conv2d_fwd_split_k_and_odd_segments(N, H, W, segs, Cout, capfd, monkeypatch):
    """test_gpu_ops.test_conv2d_fwd_split_k: the split launch (fp32 partial sums, the finish launch adds them, the bias and rounds once) and
    the unsplit launch of the same layer, each against the oracle; the two differ by the association of one fp32 sum: at most 1 %
    of the elements (a finish that kept bf16 partials or rounded before the bias would differ on a third). [200, 120]: sources that are
    no multiples of 32 channels."""
    monkeypatch.setenv("RSU_PLAN_DEBUG", "1")
    rng = np.random.RandomState(H * 7 + Cout + len(segs))
    Cin = sum(segs)
    xs = [hu.q(_rand(rng, N, H, W, c)) for c in segs]
    w = _rand(rng, 3, 3, Cin, Cout, scale=1.0 / np.sqrt(9 * Cin))
    b = _rand(rng, Cout, scale=0.1)
    xds = [hu.dev_bf16(x) for x in xs]
    wp = hu.pack_conv_fwd(w, segs if len(segs) > 1 else None)
    bd = hu.dev_f32(b)
    Ho, Wo = H - 2, W - 2
    srcs = (RsuSrc * len(segs))(*[hu.src_of(xd, H, W) for xd in xds])
    nk = int(lib().rsu_conv_splitk_ws_floats())
    kws = torch.full((nk,), float("nan"), dtype=torch.float32, device=hu.DEV)
    y = _nan(N, Ho, Wo, Cout)
    capfd.readouterr()
    call("rsu_conv2d_fwd_k", srcs, len(segs), hu.ptr(wp), hu.ptr(bd), hu.ptr(y), N, H, W, Cout, 1, 1, 0, hu.ptr(kws), nk, hu.stream())
    lines = _plan_lines(capfd)
    assert lines and " ksplit1 " not in lines[-1], lines   # the launch did split
    y1 = _nan(N, Ho, Wo, Cout)
    call("rsu_conv2d_fwd", srcs, len(segs), hu.ptr(wp), hu.ptr(bd), hu.ptr(y1), N, H, W, Cout, 1, 1, 0, hu.stream())
    split, unsplit = hu.host(y), hu.host(y1)
    ref = U.conv2d_fwd(np.concatenate(xs, axis=3), hu.q(w), b, relu=True)
    tag = "+".join(str(c) for c in segs)
    hu.assert_bf16_rounded(split, ref, "conv2d_fwd_k split-K 1x20x20x%s->%d" % (tag, Cout))
    hu.assert_bf16_rounded(unsplit, ref, "conv2d_fwd unsplit 1x20x20x%s->%d" % (tag, Cout))
    hu.assert_bf16_close(split, unsplit.astype(np.float64), "split-K vs unsplit", ulps=1.0)
    differing = float((split != unsplit).mean())
    print("split-K vs unsplit: %.5f of the elements differ" % differing)
    assert differing <= 0.01, differing


# ------------------------------------------------------------------------------------------- fused conv + pool
def test_conv2d_fwd_pool(monkeypatch):
    """test_gpu_ops.test_conv2d_fwd_pool_equals_conv_then_pool at (2, 70, 70, 64, 64), the pool folded into the conv epilogue
    (RSU_POOL_FUSED=2): the activation, the pooled tensor (a max of bf16 values: no rounding of its own) and the pooled tensor with the
    next level's dropout, q(q(pool) * mask / keep) -- the one designed second rounding, restated in the reference"""
    N, H, W, Cin, Cout = 2, 70, 70, 64, 64
    rng = np.random.RandomState(N * 7 + H + Cout)
    x = hu.q(_rand(rng, N, H, W, Cin))
    w = _rand(rng, 3, 3, Cin, Cout, scale=1.0 / np.sqrt(9 * Cin))
    b = _rand(rng, Cout, scale=0.1)
    xd, wp, bd = hu.dev_bf16(x), hu.pack_conv_fwd(w), hu.dev_f32(b)
    Ho, Wo = H - 2, W - 2
    s = (RsuSrc * 1)(hu.src_of(xd, H, W))

    def run(keep=1.0, key=0):
        y = _nan(N, Ho, Wo, Cout)
        pool = _nan(N, Ho // 2, Wo // 2, Cout)
        code = torch.full((N, Ho // 2, Wo // 2, Cout), 0xAA, dtype=torch.uint8, device=hu.DEV)
        call("rsu_conv2d_fwd_pool", s, 1, hu.ptr(wp), hu.ptr(bd), hu.ptr(y), hu.ptr(pool), hu.ptr(code), N, H, W, Cout, keep, key, 0, hu.stream())
        return hu.host(y), hu.host(pool)

    ref = U.conv2d_fwd(x, hu.q(w), b, relu=True)
    ref_pool = U.maxpool_fwd(ref)   # (rounding is monotonic: q(max) = max(q))
    monkeypatch.setenv("RSU_POOL_FUSED", "2")   # fold wherever a tile shape can
    y, pool = run()
    keep, key = 0.8, 1234
    yd, pool_d = run(keep, key)
    hu.assert_bf16_rounded(y, ref, "conv2d_fwd_pool y 2x70x70x64->64")
    hu.assert_bf16_rounded(pool, ref_pool, "conv2d_fwd_pool pooled")
    mk = U.dropout_mask(pool.shape, keep, key) * (np.float32(1) / np.float32(keep))
    hu.assert_bf16_rounded(yd, ref, "conv2d_fwd_pool y (dropout call)")
    hu.assert_bf16_rounded(pool_d, hu.q(ref_pool).astype(np.float64) * mk.astype(np.float64), "conv2d_fwd_pool pooled, dropout keep 0.8")


# ------------------------------------------------------------------------------------------- first conv
FIRST_SHAPES = [(2, 200, 203, 64, 1), (1, 64, 64, 160, 2)]


@pytest.mark.parametrize("N,H,W,Cout,dil", FIRST_SHAPES)
@pytest.mark.parametrize("gen", ["1", "0"])
def test_first_conv(N, H, W, Cout, dil, gen, monkeypatch):
    """test_gpu_ops.test_first_conv_kernel_against_oracle_and_generic_launch: k_conv_first_fwd (RSU_FIRST_GEN=1, the default) and the
    same layer on the generic implicit-GEMM kernels (0)"""
    rng = np.random.RandomState(H + Cout)
    in16 = hu.q(_rand(rng, N, H, W, 16))
    w1 = _rand(rng, 3, 3, 3, Cout, scale=0.3)
    b1 = _rand(rng, Cout, scale=0.1)
    ind, w1d, b1d = hu.dev_bf16(in16), hu.dev_f32(w1), hu.dev_f32(b1)
    pk1 = torch.zeros(lib().rsu_packed_first_bytes(Cout) // 2, dtype=torch.bfloat16, device=hu.DEV)
    call("rsu_pack_conv_first", hu.ptr(w1d), hu.ptr(pk1), Cout, hu.stream())
    monkeypatch.setenv("RSU_FIRST_GEN", gen)
    y = _nan(N, H - 2 * dil, W - 2 * dil, Cout)
    call("rsu_conv_first_fwd", hu.ptr(ind), hu.ptr(pk1), hu.ptr(b1d), hu.ptr(y), N, H, W, Cout, dil, 0, hu.stream())
    ref = U.conv2d_fwd(in16[..., 0:3], hu.q(w1), b1, dil=dil)
    hu.assert_bf16_rounded(hu.host(y), ref, "conv_first_fwd %dx%dx%d->%d dil %d RSU_FIRST_GEN=%s" % (N, H, W, Cout, dil, gen))


@pytest.mark.parametrize("N,H,W,Cout,dil", FIRST_SHAPES)
def test_colour_adjust_fused_into_the_first_conv(N, H, W, Cout, dil):
    """test_gpu_ops.test_colour_adjust_fused_into_the_first_conv_gives_the_two_launches_bits: rsu_color_conv_first_fwd against the oracle's
    conv on the device's own bf16 net0 (rsu_color_adjust_fwd: net0's rounding is not this kernel's)"""
    rng = np.random.RandomState(5 + H)
    x = rng.rand(N, H, W, 3).astype(np.float32)
    w0, b0 = _rand(rng, 3, 3, scale=0.5), _rand(rng, 3, scale=0.1)
    w1, b1 = _rand(rng, 3, 3, 3, Cout, scale=0.3), _rand(rng, Cout, scale=0.1)
    xd_, w0d, b0d, w1d, b1d = hu.dev_f32(x), hu.dev_f32(w0), hu.dev_f32(b0), hu.dev_f32(w1), hu.dev_f32(b1)
    in16 = torch.zeros((N, H, W, 16), dtype=torch.bfloat16, device=hu.DEV)
    pk1 = torch.zeros(lib().rsu_packed_first_bytes(Cout) // 2, dtype=torch.bfloat16, device=hu.DEV)
    call("rsu_pack_conv_first", hu.ptr(w1d), hu.ptr(pk1), Cout, hu.stream())
    yb = _nan(N, H - 2 * dil, W - 2 * dil, Cout)
    call("rsu_color_adjust_fwd", hu.ptr(xd_), hu.ptr(w0d), hu.ptr(b0d), hu.ptr(in16), N * H * W, 1.0, 0, hu.stream())
    call("rsu_color_conv_first_fwd", hu.ptr(xd_), hu.ptr(w0d), hu.ptr(b0d), hu.ptr(pk1), hu.ptr(b1d), hu.ptr(yb), N, H, W, Cout, dil, 0, hu.stream())
    ref = U.conv2d_fwd(hu.host(in16)[..., 0:3], hu.q(w1), b1, dil=dil)
    hu.assert_bf16_rounded(hu.host(yb), ref, "color_conv_first_fwd %dx%dx%d->%d dil %d" % (N, H, W, Cout, dil))


# ------------------------------------------------------------------------------------------- backward data
def test_conv2d_bwd_data_mask_plain_and_accumulate():
    """test_gpu_ops.test_conv2d_bwd_data at (2, 37, 41, 64, 64): with the ReLU mask, without, and accumulating onto the stored result --
    the designed second rounding q(first + g), which the op test grants 2 ulps: held to 1 ulp and the statistic here"""
    N, H, W, Cin, Cout, dil = 2, 37, 41, 64, 64, 1
    rng = np.random.RandomState(Cin + Cout * 3 + W)
    Ho, Wo = H - 2 * dil, W - 2 * dil
    dz = hu.q(_rand(rng, N, Ho, Wo, Cout))
    w = _rand(rng, 3, 3, Cin, Cout, scale=1.0 / np.sqrt(9 * Cout))
    yprev = hu.q(np.maximum(_rand(rng, N, H, W, Cin), 0))
    wp = hu.pack_conv_bwd(w)
    dzd, yd = hu.dev_bf16(dz), hu.dev_bf16(yprev)
    dx = _nan(N, H, W, Cin)
    call("rsu_conv2d_bwd_data", hu.ptr(dzd), hu.ptr(wp), hu.ptr(dx), hu.ptr(yd), 0, N, H, W, Cin, 0, Cin, Cout, dil, 0, hu.stream())
    g = U.conv2d_bwd_data(dz, hu.q(w), (H, W), dil=dil)
    hu.assert_bf16_rounded(hu.host(dx), U.relu_bwd(yprev, g), "conv2d_bwd_data 2x37x41x64<-64 ReLU mask")
    dx2 = torch.zeros((N, H, W, Cin), dtype=torch.bfloat16, device=hu.DEV)
    call("rsu_conv2d_bwd_data", hu.ptr(dzd), hu.ptr(wp), hu.ptr(dx2), None, 0, N, H, W, Cin, 0, Cin, Cout, dil, 0, hu.stream())
    first = hu.host(dx2).copy()
    hu.assert_bf16_rounded(first, g, "conv2d_bwd_data 2x37x41x64<-64 no mask")
    call("rsu_conv2d_bwd_data", hu.ptr(dzd), hu.ptr(wp), hu.ptr(dx2), None, 1, N, H, W, Cin, 0, Cin, Cout, dil, 0, hu.stream())
    hu.assert_bf16_rounded(hu.host(dx2), first.astype(np.float64) + g.astype(np.float64), "conv2d_bwd_data 2x37x41x64<-64 accumulate")


def test_conv2d_bwd_data_source_slice():
    """test_gpu_ops.test_conv2d_bwd_data_source_slice (N = 2: 10,000 elements per slice)"""
    rng = np.random.RandomState(9)
    N, H, Cin, Cout = 2, 20, 48, 32
    dz = hu.q(_rand(rng, N, H - 2, H - 2, Cout))
    w = _rand(rng, 3, 3, Cin, Cout, scale=0.1)
    full = U.conv2d_bwd_data(dz, hu.q(w), (H, H))
    dzd = hu.dev_bf16(dz)
    for off, cnt in [(0, 16), (16, 16), (32, 16)]:
        wp = hu.pack_conv_bwd(w, off, cnt)
        dx = _nan(N, H, H, cnt)
        call("rsu_conv2d_bwd_data", hu.ptr(dzd), hu.ptr(wp), hu.ptr(dx), None, 0, N, H, H, cnt, 0, cnt, Cout, 1, 0, hu.stream())
        hu.assert_bf16_rounded(hu.host(dx), np.ascontiguousarray(full[..., off:off + cnt]), "conv2d_bwd_data source slice %d..%d of 48" % (off, off + cnt))


def test_conv2d_bwd_data_split_k(capfd, monkeypatch):
    """test_gpu_ops.test_conv2d_bwd_data_split_k at (1, 20, 20, 512, 512): the finish launch applies the mask and rounds once"""
    monkeypatch.setenv("RSU_PLAN_DEBUG", "1")
    N, H, W, Cin, Cout = 1, 20, 20, 512, 512
    rng = np.random.RandomState(Cin + Cout * 3 + W)
    Ho, Wo = H - 2, W - 2
    dz = hu.q(_rand(rng, N, Ho, Wo, Cout))
    w = _rand(rng, 3, 3, Cin, Cout, scale=1.0 / np.sqrt(9 * Cout))
    yprev = hu.q(np.maximum(_rand(rng, N, H, W, Cin), 0))
    wp = hu.pack_conv_bwd(w)
    dzd, yd = hu.dev_bf16(dz), hu.dev_bf16(yprev)
    nk = int(lib().rsu_conv_splitk_ws_floats())
    kws = torch.full((nk,), float("nan"), dtype=torch.float32, device=hu.DEV)
    g = U.conv2d_bwd_data(dz, hu.q(w), (H, W))
    for mask in (yd, None):
        dx = _nan(N, H, W, Cin)
        capfd.readouterr()
        call("rsu_conv2d_bwd_data_k", hu.ptr(dzd), hu.ptr(wp), hu.ptr(dx), hu.ptr(mask) if mask is not None else None, 0, N, H, W, Cin, 0, Cin, Cout, 1, 0,
             hu.ptr(kws), nk, hu.stream())
        lines = _plan_lines(capfd)
        assert lines and " ksplit1 " not in lines[-1], lines
        hu.assert_bf16_rounded(hu.host(dx), U.relu_bwd(yprev, g) if mask is not None else g,
                               "conv2d_bwd_data_k split-K 1x20x20x512<-512 %s" % ("ReLU mask" if mask is not None else "no mask"))


@forced
def test_conv2d_bwd_data_every_forced_shape(cfg, gen, monkeypatch):
    x, w, b, dz, _, ref_dx = _cfg_case()
    N, H, W, Cin = x.shape
    Cout = w.shape[3]
    assert Cin % 32 == 0
    _force(monkeypatch, cfg, gen)
    xd, dzd, wb = hu.dev_bf16(x), hu.dev_bf16(dz), hu.pack_conv_bwd(w, 0, Cin)
    dx = _nan(N, H, W, Cin)
    call("rsu_conv2d_bwd_data", hu.ptr(dzd), hu.ptr(wb), hu.ptr(dx), hu.ptr(xd), 0, N, H, W, Cin, 0, Cin, Cout, 1, 0, hu.stream())
    hu.assert_bf16_rounded(hu.host(dx), ref_dx, "conv2d_bwd_data 1x70x75x64<-192 RSU_FWD2_CFG=%d RSU_FWD_GEN=%d" % (cfg, gen))


# ------------------------------------------------------------------------------------------- transposed conv, dropout
@pytest.mark.parametrize("N,H,W,Cin,Cout", [(2, 52, 50, 96, 96), (1, 28, 28, 256, 128)])
@pytest.mark.parametrize("gen", ["2", "1"])
def test_convT_fwd_bwd_data_and_dropout(N, H, W, Cin, Cout, gen, monkeypatch):
    """test_gpu_ops.test_convT / test_gpu_cfg_matrix.test_convT_both_generations_against_the_oracle: igemm_ct (RSU_CT_GEN=2) and igemm_fwd2's
    tap launches (1): forward, backward-data with the ReLU mask, and backward-data behind the dropout (the dropped tensor as mask source,
    1/keep applied by a second pass to the stored bf16 gradient: a designed second rounding, restated in the reference); rsu_dropout_fwd
    itself on the way"""
    rng = np.random.RandomState(Cin + H)
    x = hu.q(np.maximum(_rand(rng, N, H, W, Cin), 0))
    K = _rand(rng, 2, 2, Cout, Cin, scale=1.0 / np.sqrt(Cin))
    b = _rand(rng, Cout, scale=0.1)
    seg = (ctypes.c_int * 1)(Cin)
    pf = torch.zeros(4 * lib().rsu_packed_bytes(1, Cout, seg, 1) // 2, dtype=torch.bfloat16, device=hu.DEV)
    seg2 = (ctypes.c_int * 1)(Cout)
    pb = torch.zeros(lib().rsu_packed_bytes(4, Cin, seg2, 1) // 2, dtype=torch.bfloat16, device=hu.DEV)
    Kd = hu.dev_f32(K)
    call("rsu_pack_convT_fwd", hu.ptr(Kd), hu.ptr(pf), Cin, Cout, hu.stream())
    call("rsu_pack_convT_bwd", hu.ptr(Kd), hu.ptr(pb), Cin, Cout, hu.stream())
    monkeypatch.setenv("RSU_CT_GEN", gen)
    tag = "%dx%dx%dx%d->%d RSU_CT_GEN=%s" % (N, H, W, Cin, Cout, gen)
    xd, bd = hu.dev_bf16(x), hu.dev_f32(b)
    y = _nan(N, 2 * H, 2 * W, Cout)
    call("rsu_convT2x2_fwd", hu.ptr(xd), hu.ptr(pf), hu.ptr(bd), hu.ptr(y), N, H, W, Cin, Cout, 0, hu.stream())
    hu.assert_bf16_rounded(hu.host(y), U.convT_fwd(x, hu.q(K), b), "convT2x2_fwd " + tag)
    dy = hu.q(_rand(rng, N, 2 * H, 2 * W, Cout, scale=0.1))
    dyd = hu.dev_bf16(dy)
    dx = _nan(N, H, W, Cin)
    call("rsu_convT2x2_bwd_data", hu.ptr(dyd), hu.ptr(pb), hu.ptr(dx), hu.ptr(xd), 1.0, N, H, W, Cin, Cout, 0, hu.stream())
    rdx = U.convT_bwd(x, hu.q(K), dy)[0]
    first = hu.host(dx).copy()
    hu.assert_bf16_rounded(first, U.relu_bwd(x, rdx), "convT2x2_bwd_data " + tag)
    keep, key = 0.8, 0x5EED0001
    inv = np.float32(1) / np.float32(keep)
    xdrop = _nan(N, H, W, Cin)
    call("rsu_dropout_fwd", hu.ptr(xd), hu.ptr(xdrop), x.size, keep, key, hu.stream())
    m = U.dropout_mask(x.shape, keep, key)
    if gen == "2":
        hu.assert_bf16_rounded(hu.host(xdrop), x.astype(np.float64) * m * np.float64(inv), "dropout_fwd %dx%dx%dx%d keep 0.8" % (N, H, W, Cin))
    dx = _nan(N, H, W, Cin)
    call("rsu_convT2x2_bwd_data", hu.ptr(dyd), hu.ptr(pb), hu.ptr(dx), hu.ptr(xdrop), float(inv), N, H, W, Cin, Cout, 0, hu.stream())
    # the designed second rounding (rsu.h): the kernel stores q(sum) and a second pass multiplies the stored tensor
    # by 1/keep -> q(q(sum) / keep). (Against the once-rounded q(sum / keep) this case measures mismatch 0.27, bias -0.006.) The first
    # rounding is the device's own, just checked above, as in the accumulate case: a legitimate 1-ulp flip of it is up to 2 ulps behind
    # the scale (2 of 499,200 elements against the oracle's q(sum)).
    ref = np.where(m > 0, first.astype(np.float64) * np.float64(inv), 0.0)
    hu.assert_bf16_rounded(hu.host(dx), ref, "convT2x2_bwd_data with dropout " + tag)


# ------------------------------------------------------------------------------------------- the gradient junction
def _up2(a):
    return np.repeat(np.repeat(a, 2, axis=1), 2, axis=2)


@pytest.mark.parametrize("use_pool,use_skip,dropout", [(1, 1, 0), (1, 0, 0), (0, 1, 0), (1, 1, 1)], ids=["both", "pool", "skip", "both-dropout"])
def test_pool_skip_relu_bwd(use_pool, use_skip, dropout):
    """test_gpu_ops.test_maxpool_fwd_and_junction_bwd at (30, 26, 16), N = 4: rsu_pool_skip_relu_bwd and its _code twin. The pool routes a
    gradient to one element in four and the skip covers the centre only, so most of dz is zero BY STRUCTURE: those elements must be
    exactly zero, and the statistic (its 10,000 elements and 35 % included) is taken over the support -- the routed elements, the
    centre. A sum of two bf16 values is exact in fp32: without dropout every element must match."""
    N, H, W, C = 4, 30, 26, 16
    rng = np.random.RandomState(H + C)
    x = hu.q(np.maximum(_rand(rng, N, H, W, C), 0))
    x[0, :4, :4, :] = x[0, 0, 0, :]  # force ties (incl. zeros) in a corner
    keep, key = 0.8, 0x1234ABCD
    kp = keep if dropout else 1.0
    Hs, Ws = H - 4, W - 6
    dpool = hu.q(_rand(rng, N, H // 2, W // 2, C))
    dskip = hu.q(_rand(rng, N, Hs, Ws, C))
    xd, dpd, dsd = hu.dev_bf16(x), hu.dev_bf16(dpool), hu.dev_bf16(dskip)
    dz = _nan(N, H, W, C)
    call("rsu_pool_skip_relu_bwd", hu.ptr(xd), hu.ptr(dpd) if use_pool else None, hu.ptr(dsd) if use_skip else None, hu.ptr(dz), N, H, W, C, Hs, Ws,
         kp, key, hu.stream())
    code = torch.full((N, H // 2, W // 2, C), 255, dtype=torch.uint8, device=hu.DEV)
    y2 = _nan(N, H // 2, W // 2, C)
    call("rsu_maxpool2x2_fwd_code", hu.ptr(xd), hu.ptr(y2), hu.ptr(code), N, H, W, C, kp, key, hu.stream())
    dz2 = _nan(N, H, W, C)
    call("rsu_pool_skip_relu_bwd_code", None, hu.ptr(code), hu.ptr(dpd) if use_pool else None, hu.ptr(dsd) if use_skip else None, hu.ptr(dz2), N, H, W, C,
         Hs, Ws, kp, key, hu.stream())
    g = np.zeros(x.shape, np.float64)
    support = np.zeros(x.shape, bool)
    if use_pool:
        route = U.maxpool_bwd(x, np.ones(dpool.shape, np.float32))   # 1 at each window's first maximum
        mk = (U.dropout_mask(dpool.shape, keep, key) * (np.float32(1) / np.float32(keep))).astype(np.float64) if dropout else np.ones(dpool.shape)
        g += route * _up2(dpool.astype(np.float64) * mk)
        support |= (route != 0) & (_up2(mk) != 0)
    if use_skip:
        g += U.center_pad_like(dskip, x.shape)
        support |= U.center_pad_like(np.ones_like(dskip), x.shape) != 0
    ref = np.where(x > 0, g, 0.0)
    assert not ref[~support].any()
    what = "pool=%d skip=%d keep %g" % (use_pool, use_skip, kp)
    for name, t in (("pool_skip_relu_bwd", dz), ("pool_skip_relu_bwd_code", dz2)):
        got = hu.host(t)
        assert not np.isnan(got).any() and not got[~support].any(), name + ": something outside the support"
        mismatch, _, _ = hu.assert_bf16_rounded(got[support], ref[support], "%s 4x30x26x16 %s" % (name, what))
        if not dropout:
            assert mismatch == 0.0, (name, what, mismatch)


# ------------------------------------------------------------------------------------------- the heads' dact
class _HeadOut:
    def __init__(self, C):
        z = lambda *s, dtype=torch.float32: torch.zeros(s, dtype=dtype, device=hu.DEV)  # noqa: E731
        self.prob_a, self.sums, self.prob = z(NPIX), z(3), z(NPIX)
        self.dact = _nan(NPIX, C)
        self.dw, self.db, self.loss, self.wsum = z(C, 2), z(2), z(1), z(1)


@pytest.mark.parametrize("C", [64, 16])
def test_head_dact(C):
    """test_gpu_ops.test_head"""
    _, act, w, b, labels = _inputs(C)
    ad, wd, bd = hu.dev_bf16(act), hu.dev_f32(w), hu.dev_f32(b)
    o = _HeadOut(C)
    ws = torch.zeros(lib().rsu_head_ws_floats(NPIX, C), dtype=torch.float32, device=hu.DEV)
    lab = torch.from_numpy(labels).to(hu.DEV)
    inv = 1.0 / (2 * NPIX)
    call("rsu_head_fwd_bwd", hu.ptr(ad), hu.ptr(wd), hu.ptr(bd), hu.ptr(lab), hu.ptr(o.prob), hu.ptr(o.loss), hu.ptr(o.dact), hu.ptr(o.dw), hu.ptr(o.db),
         hu.ptr(ws), NPIX, C, inv, hu.stream())
    ref = Ref(act, w, b, labels, None, None, inv, lam=0.0)
    hu.assert_bf16_rounded(hu.host(o.dact), ref.dact, "head_fwd_bwd dact C=%d" % C)


@pytest.mark.parametrize("C", [64, 16])
def test_weighted_head_dact(C):
    """test_gpu_weighted_loss.test_weighted_head_against_reference, mode "both" (class weights and a weight map with zeros)"""
    rng, act, w, b, labels = _inputs(C)
    class_w, pixel_w = (0.6, 2.5), _weight_map(rng)
    o = _HeadOut(C)
    ws = torch.zeros(lib().rsu_head_w_ws_floats(NPIX, C), dtype=torch.float32, device=hu.DEV)
    ad, wd, bd, lab = hu.dev_bf16(act), hu.dev_f32(w), hu.dev_f32(b), _dev_labels(labels)
    cw, pw = hu.dev_f32(np.asarray(class_w, np.float32)), hu.dev_f32(pixel_w)
    inv = 1.0 / (2 * NPIX)
    call("rsu_head_fwd_bwd_w", hu.ptr(ad), hu.ptr(wd), hu.ptr(bd), hu.ptr(lab), hu.ptr(cw), hu.ptr(pw), hu.ptr(o.prob), hu.ptr(o.loss),
         hu.ptr(o.wsum), hu.ptr(o.dact), hu.ptr(o.dw), hu.ptr(o.db), hu.ptr(ws), NPIX, C, inv, hu.stream())
    ref = Ref(act, w, b, labels, class_w, pixel_w, inv, lam=0.0)
    hu.assert_bf16_rounded(hu.host(o.dact), ref.dact, "head_fwd_bwd_w dact C=%d" % C)


@pytest.mark.parametrize("C", [64, 16])
def test_dice_head_dact(C):
    """test_gpu_dice_loss.test_dice_gradients_against_float64_autograd, mode "plain" with class weights"""
    _, act, w, b, labels = _inputs(C)
    class_w = (0.6, 2.5)
    o = _HeadOut(C)
    ws = torch.zeros(lib().rsu_head_dice_ws_floats(NPIX, C), dtype=torch.float32, device=hu.DEV)
    ad, wd, bd, lab = hu.dev_bf16(act), hu.dev_f32(w), hu.dev_f32(b), _dev_labels(labels)
    cw = hu.dev_f32(np.asarray(class_w, np.float32))
    inv = 1.0 / (2 * NPIX)
    call("rsu_head_dice_sums", hu.ptr(ad), hu.ptr(wd), hu.ptr(bd), hu.ptr(lab), None, hu.ptr(o.prob_a), hu.ptr(o.sums), hu.ptr(ws), NPIX, C, hu.stream())
    call("rsu_head_fwd_bwd_dice", hu.ptr(ad), hu.ptr(wd), hu.ptr(bd), hu.ptr(lab), hu.ptr(cw), None, hu.ptr(o.sums), LAM, SMOOTH,
         hu.ptr(o.prob), hu.ptr(o.loss), hu.ptr(o.wsum), hu.ptr(o.dact), hu.ptr(o.dw), hu.ptr(o.db), hu.ptr(ws), NPIX, C, inv, hu.stream())
    ref = Ref(act, w, b, labels, class_w, None, inv)
    hu.assert_bf16_rounded(hu.host(o.dact), ref.dact, "head_fwd_bwd_dice dact C=%d" % C)


# ------------------------------------------------------------------------------------------- the bf16 weight copies
@pytest.mark.parametrize("optimizer", ["momentum", "adam"])
def test_repacked_weight_copies(optimizer):
    """The packed bf16 copies that rsu_update_table_run / rsu_update_table_run_adam write from the new fp32 weights are otherwise checked
    only through use. The (3, 16) net of test_gpu_soak.test_fused_update_equals_momentum_then_repack after one step: its level-0
    conv2 (16 -> 16, a zero-padded K chunk) run on the re-packed buffers against the oracle with q(w_new) -- a copy that was truncated,
    or packed from the old weights, moves a large share of the outputs."""
    from road_segmentation_unet_amd.unet import UNet
    m = UNet(3, 16, True, 2, 60, seed=17, training=True, optimizer=optimizer)
    name = "conv_0/conv2"
    w_old = m.w[name + "/kernel"].detach().cpu().numpy().copy()
    _batch(m)
    m.forward_device()
    m.backward_device(1.0 / (2 * 60 * 60))
    if optimizer == "momentum":
        m.apply_momentum(0.05, 0.9)
    else:
        m.apply_adam(1e-3)
    torch.cuda.synchronize()
    w_new = m.w[name + "/kernel"].detach().cpu().numpy().copy()
    b_new = m.w[name + "/bias"].detach().cpu().numpy().copy()
    assert (w_new != w_old).mean() > 0.9, "the step did not move the weights"
    N, H, C = 2, m.S - 2, 16
    rng = np.random.RandomState(16)
    x = hu.q(_rand(rng, N, H, H, C))
    xd = hu.dev_bf16(x)
    y = _nan(N, H - 2, H - 2, C)
    s = (RsuSrc * 1)(hu.src_of(xd, H, H))
    call("rsu_conv2d_fwd", s, 1, hu.ptr(m.pk[name + "/kernel", "fwd"]), hu.ptr(m.w[name + "/bias"]), hu.ptr(y), N, H, H, C, 1, 1, 0, hu.stream())
    hu.assert_bf16_rounded(hu.host(y), U.conv2d_fwd(x, hu.q(w_new), b_new, relu=True), "conv2d_fwd on the copy re-packed by the %s update" % optimizer)
    dz = hu.q(_rand(rng, N, H - 2, H - 2, C))
    dzd = hu.dev_bf16(dz)
    dx = _nan(N, H, H, C)
    call("rsu_conv2d_bwd_data", hu.ptr(dzd), hu.ptr(m.pk[name + "/kernel", "bwd", 0]), hu.ptr(dx), None, 0, N, H, H, C, 0, C, C, 1, 0, hu.stream())
    hu.assert_bf16_rounded(hu.host(dx), U.conv2d_bwd_data(dz, hu.q(w_new), (H, H)), "conv2d_bwd_data on the copy re-packed by the %s update" % optimizer)
