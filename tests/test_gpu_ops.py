"""-m gpu: op-level parity of the HIP kernels, called through the C ABI (include/rsu.h), against the CPU oracle on the
same seeded, bf16-rounded inputs. Tolerances (stated in hiputil.assert_bf16_close): 1 bfloat16 ulp relative (2^-7)
+ 2e-5*max|ref| for bf16 outputs; rtol 1e-4 (+1e-5*max|ref|) for float32 outputs accumulated from bf16 data."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tiler_oracle as T  # noqa: E402
from oracle import unet_oracle as U  # noqa: E402
from tests import hiputil as hu  # noqa: E402
from road_segmentation_unet_amd._lib import RsuSrc, call, lib  # noqa: E402


def _rand(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


# ------------------------------------------------------------------------------------------- conv forward
CONV_SHAPES = [
    # N, H, W, Cin, Cout, dil
    (1, 12, 12, 32, 64, 1),
    (2, 37, 41, 64, 64, 1),
    (1, 30, 30, 16, 16, 1),
    (1, 40, 36, 96, 128, 2),
    (1, 70, 75, 64, 192, 1),
    (2, 20, 20, 128, 256, 1),
    (1, 150, 140, 64, 64, 1),
    (1, 26, 26, 256, 128, 2),
    (1, 8, 8, 1536, 1024, 1),  # > 256 weight tiles: fewer grid.z splits than wave groups (workspace sizing)
]


@pytest.mark.parametrize("N,H,W,Cin,Cout,dil", CONV_SHAPES)
@pytest.mark.parametrize("relu", [1, 0])
def test_conv2d_fwd(N, H, W, Cin, Cout, dil, relu):
    rng = np.random.RandomState(Cin * 7 + Cout + H)
    x = hu.q(_rand(rng, N, H, W, Cin))
    w = _rand(rng, 3, 3, Cin, Cout, scale=1.0 / np.sqrt(9 * Cin))
    b = _rand(rng, Cout, scale=0.1)
    xd = hu.dev_bf16(x)
    wp = hu.pack_conv_fwd(w)
    bd = hu.dev_f32(b)
    Ho, Wo = H - 2 * dil, W - 2 * dil
    y = torch.full((N, Ho, Wo, Cout), float("nan"), dtype=torch.bfloat16, device=hu.DEV)
    s = (RsuSrc * 1)(hu.src_of(xd, H, W))
    call("rsu_conv2d_fwd", s, 1, hu.ptr(wp), hu.ptr(bd), hu.ptr(y), N, H, W, Cout, dil, relu, 0, hu.stream())
    ref = U.conv2d_fwd(x, hu.q(w), b, dil=dil, relu=bool(relu))
    hu.assert_bf16_close(hu.host(y), ref, "conv2d_fwd")


def test_conv2d_fwd_three_cropped_sources():
    """virtual crop+concat of unet.py:70-85: [skip (cropped), dilated skip (cropped), up]"""
    rng = np.random.RandomState(5)
    N, h, w = 2, 22, 26
    a = hu.q(_rand(rng, N, 34, 38, 32))
    bsrc = hu.q(_rand(rng, N, 28, 30, 32))
    c = hu.q(_rand(rng, N, h, w, 32))
    W = _rand(rng, 3, 3, 96, 64, scale=0.05)
    bias = _rand(rng, 64, scale=0.1)
    ad, bd_, cd = hu.dev_bf16(a), hu.dev_bf16(bsrc), hu.dev_bf16(c)
    wp = hu.pack_conv_fwd(W, [32, 32, 32])
    y = torch.zeros((N, h - 2, w - 2, 64), dtype=torch.bfloat16, device=hu.DEV)
    srcs = (RsuSrc * 3)(hu.src_of(ad, h, w), hu.src_of(bd_, h, w), hu.src_of(cd, h, w))
    biasd = hu.dev_f32(bias)
    call("rsu_conv2d_fwd", srcs, 3, hu.ptr(wp), hu.ptr(biasd), hu.ptr(y), N, h, w, 64, 1, 1, 0, hu.stream())
    cat = np.concatenate([U.center_crop(a, h, w), U.center_crop(bsrc, h, w), c], axis=3)
    ref = U.conv2d_fwd(cat, hu.q(W), bias, relu=True)
    hu.assert_bf16_close(hu.host(y), ref, "conv2d_fwd 3 sources")


def test_conv2d_fwd_odd_channel_segments():
    """channel counts that are multiples of 8 but not of 32 (root_size 16 / 8 networks): K segments are zero-padded"""
    rng = np.random.RandomState(6)
    N, h = 1, 18
    a, c = hu.q(_rand(rng, N, 24, 24, 16)), hu.q(_rand(rng, N, h, h, 16))
    W = _rand(rng, 3, 3, 32, 16, scale=0.1)
    wp = hu.pack_conv_fwd(W, [16, 16])
    y = torch.zeros((N, h - 2, h - 2, 16), dtype=torch.bfloat16, device=hu.DEV)
    ad, cd = hu.dev_bf16(a), hu.dev_bf16(c)
    srcs = (RsuSrc * 2)(hu.src_of(ad, h, h), hu.src_of(cd, h, h))
    call("rsu_conv2d_fwd", srcs, 2, hu.ptr(wp), None, hu.ptr(y), N, h, h, 16, 1, 1, 0, hu.stream())
    ref = U.conv2d_fwd(np.concatenate([U.center_crop(a, h, h), c], axis=3), hu.q(W), None, relu=True)
    hu.assert_bf16_close(hu.host(y), ref, "conv2d_fwd 16+16")


# ------------------------------------------------------------------------------------------- split-K (rsu_conv2d_*_k)
def _plan_lines(capfd):
    return [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[plan fwd2]")]


SPLITK_SHAPES = [
    # N, H, W, srcs (channels), Cout: few pixels, long reductions -- the deep levels of configs 3 / 4 at one patch per step
    (1, 20, 20, [512], 512),
    (1, 22, 18, [256, 256, 128], 256),   # three concat sources, a slice boundary inside a source and slices that start in the 2nd / 3rd
    (2, 12, 12, [1024], 256),
    (1, 20, 20, [200, 120], 128),        # sources that are not multiples of 32 channels (partial last chunks inside slices)
]


@pytest.mark.parametrize("N,H,W,segs,Cout", SPLITK_SHAPES)
def test_conv2d_fwd_split_k(N, H, W, segs, Cout, capfd, monkeypatch):
    """rsu_conv2d_fwd_k with a workspace: the planner cuts the reduction of these few-pixel layers into slices (checked on its debug
    line), the finish launch sums them in slice order -> against the oracle (the op tolerance) and against the unsplit launch (equal up to
    the association of one fp32 sum: at most a rounding-boundary flip of 1 bf16 ulp), repeatable bit for bit"""
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
    outs = []
    for rep in range(2):
        y = torch.full((N, Ho, Wo, Cout), float("nan"), dtype=torch.bfloat16, device=hu.DEV)
        capfd.readouterr()
        call("rsu_conv2d_fwd_k", srcs, len(segs), hu.ptr(wp), hu.ptr(bd), hu.ptr(y), N, H, W, Cout, 1, 1, 0, hu.ptr(kws), nk, hu.stream())
        lines = _plan_lines(capfd)
        assert lines and " ksplit1 " not in lines[-1], lines   # the launch did split
        outs.append(hu.host(y))
    np.testing.assert_array_equal(outs[0], outs[1])
    ref = U.conv2d_fwd(np.concatenate(xs, axis=3), hu.q(w), b, relu=True)
    hu.assert_bf16_close(outs[0], ref, "conv2d_fwd split-K")
    y1 = torch.full((N, Ho, Wo, Cout), float("nan"), dtype=torch.bfloat16, device=hu.DEV)
    call("rsu_conv2d_fwd", srcs, len(segs), hu.ptr(wp), hu.ptr(bd), hu.ptr(y1), N, H, W, Cout, 1, 1, 0, hu.stream())
    hu.assert_bf16_close(outs[0], hu.host(y1).astype(np.float64), "split-K vs unsplit", ulps=1.0)
    assert (outs[0] != hu.host(y1)).mean() <= 0.01   # (a correct fp32 finish: ~3e-4; partial sums kept in bf16: a third. tests/test_gpu_rounding.py)


@pytest.mark.parametrize("H,Cin,Cout", [(32, 512, 1024), (30, 1024, 1024), (20, 1024, 2048)])
def test_split_k_plan_depends_on_the_batch_and_by_how_much(H, Cin, Cout, capfd, monkeypatch):
    """The slice count of a split launch is a function of the geometry INCLUDING the batch (rsu.h, rsu_conv2d_fwd_k): the deep layers of c2 /
    c4 (level 4 at 32 / 30 pixels, level 5 at 20) cut their reduction into more slices at N = 1 than at N = 4. Pinned here, per layer: four
    copies of one image give, image by image, the N = 1 result up to the association of one fp32 sum -- at most 1 bf16 ulp on a small
    fraction of the elements -- and both stay inside the op tolerance against the oracle. (The per-image rule that would make them equal bit
    for bit cost the N = 4 step 12-14 %: profiles/r05/abenv_perimg_c2.txt.)"""
    monkeypatch.setenv("RSU_PLAN_DEBUG", "1")
    rng = np.random.RandomState(H + Cin + Cout)
    x1 = hu.q(_rand(rng, 1, H, H, Cin))
    w = _rand(rng, 3, 3, Cin, Cout, scale=1.0 / np.sqrt(9 * Cin))
    b = _rand(rng, Cout, scale=0.1)
    wp, bd = hu.pack_conv_fwd(w), hu.dev_f32(b)
    nk = int(lib().rsu_conv_splitk_ws_floats())
    kws = torch.full((nk,), float("nan"), dtype=torch.float32, device=hu.DEV)
    outs, splits = {}, {}
    for N in (1, 4):
        xd = hu.dev_bf16(np.concatenate([x1] * N))
        y = torch.full((N, H - 2, H - 2, Cout), float("nan"), dtype=torch.bfloat16, device=hu.DEV)
        srcs = (RsuSrc * 1)(hu.src_of(xd, H, H))
        capfd.readouterr()
        call("rsu_conv2d_fwd_k", srcs, 1, hu.ptr(wp), hu.ptr(bd), hu.ptr(y), N, H, H, Cout, 1, 1, 0, hu.ptr(kws), nk, hu.stream())
        line = _plan_lines(capfd)[-1]
        splits[N] = int(line.split(" ksplit")[1].split()[0])
        outs[N] = hu.host(y)
    assert splits[1] > splits[4] >= 1, splits   # (if the rule ever becomes batch-independent this test should turn into a bit-equality test)
    ref = U.conv2d_fwd(x1, hu.q(w), b, relu=True)
    hu.assert_bf16_close(outs[1], ref, "N = 1")
    for n in range(4):
        np.testing.assert_array_equal(outs[4][n], outs[4][0])
    hu.assert_bf16_close(outs[4][:1], ref, "N = 4")
    hu.assert_bf16_close(outs[4][:1], outs[1].astype(np.float64), "N = 4 vs N = 1", ulps=1.0)
    assert (outs[4][:1] != outs[1]).mean() <= 0.01


@pytest.mark.parametrize("N,H,W,Cin,Cout", [(1, 20, 20, 512, 512), (2, 14, 14, 256, 1024)])
def test_conv2d_bwd_data_split_k(N, H, W, Cin, Cout, capfd, monkeypatch):
    """rsu_conv2d_bwd_data_k: split reduction with the ReLU mask applied by the finish launch"""
    monkeypatch.setenv("RSU_PLAN_DEBUG", "1")
    rng = np.random.RandomState(Cin + Cout * 3 + W)
    Ho, Wo = H - 2, W - 2
    dz = hu.q(_rand(rng, N, Ho, Wo, Cout))
    w = _rand(rng, 3, 3, Cin, Cout, scale=1.0 / np.sqrt(9 * Cout))
    yprev = hu.q(np.maximum(_rand(rng, N, H, W, Cin), 0))
    wp = hu.pack_conv_bwd(w)
    dzd, yd = hu.dev_bf16(dz), hu.dev_bf16(yprev)
    nk = int(lib().rsu_conv_splitk_ws_floats())
    kws = torch.full((nk,), float("nan"), dtype=torch.float32, device=hu.DEV)
    for mask in (yd, None):
        dx = torch.full((N, H, W, Cin), float("nan"), dtype=torch.bfloat16, device=hu.DEV)
        capfd.readouterr()
        call("rsu_conv2d_bwd_data_k", hu.ptr(dzd), hu.ptr(wp), hu.ptr(dx), hu.ptr(mask) if mask is not None else None, 0, N, H, W, Cin, 0, Cin, Cout, 1, 0,
             hu.ptr(kws), nk, hu.stream())
        lines = _plan_lines(capfd)
        assert lines and " ksplit1 " not in lines[-1], lines
        g = U.conv2d_bwd_data(dz, hu.q(w), (H, W))
        hu.assert_bf16_close(hu.host(dx), U.relu_bwd(yprev, g) if mask is not None else g, "conv2d_bwd_data split-K")


# ------------------------------------------------------------------------------------------- conv backward data
@pytest.mark.parametrize("N,H,W,Cin,Cout,dil", CONV_SHAPES[:6])
def test_conv2d_bwd_data(N, H, W, Cin, Cout, dil):
    rng = np.random.RandomState(Cin + Cout * 3 + W)
    Ho, Wo = H - 2 * dil, W - 2 * dil
    dz = hu.q(_rand(rng, N, Ho, Wo, Cout))
    w = _rand(rng, 3, 3, Cin, Cout, scale=1.0 / np.sqrt(9 * Cout))
    yprev = hu.q(np.maximum(_rand(rng, N, H, W, Cin), 0))
    wp = hu.pack_conv_bwd(w)
    dzd, yd = hu.dev_bf16(dz), hu.dev_bf16(yprev)
    dx = torch.full((N, H, W, Cin), float("nan"), dtype=torch.bfloat16, device=hu.DEV)
    call("rsu_conv2d_bwd_data", hu.ptr(dzd), hu.ptr(wp), hu.ptr(dx), hu.ptr(yd), 0, N, H, W, Cin, 0, Cin, Cout, dil, 0, hu.stream())
    ref = U.relu_bwd(yprev, U.conv2d_bwd_data(dz, hu.q(w), (H, W), dil=dil))
    hu.assert_bf16_close(hu.host(dx), ref, "conv2d_bwd_data+relu mask")
    # no mask, then accumulate a second time: dx = q(q(g) + g)
    dx2 = torch.zeros((N, H, W, Cin), dtype=torch.bfloat16, device=hu.DEV)
    call("rsu_conv2d_bwd_data", hu.ptr(dzd), hu.ptr(wp), hu.ptr(dx2), None, 0, N, H, W, Cin, 0, Cin, Cout, dil, 0, hu.stream())
    g = U.conv2d_bwd_data(dz, hu.q(w), (H, W), dil=dil)
    hu.assert_bf16_close(hu.host(dx2), g, "conv2d_bwd_data")
    first = hu.host(dx2).copy()
    call("rsu_conv2d_bwd_data", hu.ptr(dzd), hu.ptr(wp), hu.ptr(dx2), None, 1, N, H, W, Cin, 0, Cin, Cout, dil, 0, hu.stream())
    hu.assert_bf16_close(hu.host(dx2), first.astype(np.float64) + g, "conv2d_bwd_data accumulate")   # q(stored + sum): one more rounding of an fp32 value


def test_conv2d_bwd_data_source_slice():
    """backward towards one concat source: its own weight pack (rows ci_off..ci_off+cnt of the kernel)"""
    rng = np.random.RandomState(9)
    N, H, Cin, Cout = 1, 20, 48, 32
    dz = hu.q(_rand(rng, N, H - 2, H - 2, Cout))
    w = _rand(rng, 3, 3, Cin, Cout, scale=0.1)
    full = U.conv2d_bwd_data(dz, hu.q(w), (H, H))
    for off, cnt in [(0, 16), (16, 16), (32, 16)]:
        wp = hu.pack_conv_bwd(w, off, cnt)
        dx = torch.zeros((N, H, H, cnt), dtype=torch.bfloat16, device=hu.DEV)
        dzd = hu.dev_bf16(dz)
        call("rsu_conv2d_bwd_data", hu.ptr(dzd), hu.ptr(wp), hu.ptr(dx), None, 0, N, H, H, cnt, 0, cnt, Cout, 1, 0, hu.stream())
        hu.assert_bf16_close(hu.host(dx), full[..., off:off + cnt], "bwd_data slice %d" % off)


# ------------------------------------------------------------------------------------------- conv backward weight
@pytest.mark.parametrize("N,H,W,Cin,Cout,dil", CONV_SHAPES)
def test_conv2d_bwd_weight_and_bias(N, H, W, Cin, Cout, dil):
    rng = np.random.RandomState(Cin * 3 + Cout + H)
    Ho, Wo = H - 2 * dil, W - 2 * dil
    x = hu.q(_rand(rng, N, H, W, Cin))
    dz = hu.q(_rand(rng, N, Ho, Wo, Cout, scale=0.1))
    xd, dzd = hu.dev_bf16(x), hu.dev_bf16(dz)
    dw = torch.full((3, 3, Cin, Cout), float("nan"), dtype=torch.float32, device=hu.DEV)
    db = torch.zeros(Cout, dtype=torch.float32, device=hu.DEV)
    nws = max(lib().rsu_conv2d_bwd_weight_ws_floats(Cin, Cin, Cout), lib().rsu_bias_grad_ws_floats(N * Ho * Wo, Cout))
    ws = torch.zeros(nws + 4096, dtype=torch.float32, device=hu.DEV)
    ws[nws:] = 12345.0  # guard band: the kernels must stay inside the advertised workspace
    s = hu.src_of(xd, H, W)
    db2 = torch.full((Cout,), float("nan"), dtype=torch.float32, device=hu.DEV)
    call("rsu_conv2d_bwd_weight", ctypes.byref(s), hu.ptr(dzd), hu.ptr(dw), hu.ptr(db2), hu.ptr(ws), N, Ho, Wo, Cin, 0, Cout, dil, 0, hu.stream())
    ref_dw, ref_db = U.conv2d_bwd_weight(x, dz, dil=dil)
    hu.assert_f32_close(hu.host(dw), ref_dw, "conv2d_bwd_weight")
    hu.assert_f32_close(hu.host(db2), ref_db, "bias grad fused in wgrad")
    assert bool((ws[nws:] == 12345.0).all()), "workspace overrun"
    if 256 % (Cout // 8) == 0:
        call("rsu_bias_grad", hu.ptr(dzd), hu.ptr(db), hu.ptr(ws), N * Ho * Wo, Cout, hu.stream())
        hu.assert_f32_close(hu.host(db), ref_db, "bias_grad")


@pytest.mark.parametrize("N,H,W,Cin,Cout", [(2, 30, 30, 64, 128), (1, 70, 70, 128, 256), (3, 21, 37, 72, 136), (1, 12, 140, 128, 128),
                                            (2, 10, 10, 256, 512)])
def test_pingpong_wgrad_gives_the_bits_of_igemm_wgrad(N, H, W, Cin, Cout, monkeypatch):
    """igemm_wgpp (RSU_WG_GEN=2, the default) keeps igemm_wgrad's tiles, slabs and summation order: same bits, bias sums included"""
    rng = np.random.RandomState(Cin + Cout + H)
    Ho, Wo = H - 2, W - 2
    xd = hu.dev_bf16(hu.q(_rand(rng, N, H, W, Cin)))
    dzd = hu.dev_bf16(hu.q(_rand(rng, N, Ho, Wo, Cout, scale=0.1)))
    nws = lib().rsu_conv2d_bwd_weight_ws_floats(Cin, Cin, Cout)
    out = {}
    for gen in ("1", "2"):
        monkeypatch.setenv("RSU_WG_GEN", gen)
        dw = torch.full((3, 3, Cin, Cout), float("nan"), dtype=torch.float32, device=hu.DEV)
        db = torch.full((Cout,), float("nan"), dtype=torch.float32, device=hu.DEV)
        ws = torch.zeros(nws, dtype=torch.float32, device=hu.DEV)
        s = hu.src_of(xd, H, W)
        call("rsu_conv2d_bwd_weight", ctypes.byref(s), hu.ptr(dzd), hu.ptr(dw), hu.ptr(db), hu.ptr(ws), N, Ho, Wo, Cin, 0, Cout, 1, 0, hu.stream())
        out[gen] = (hu.host(dw), hu.host(db))
    assert np.array_equal(out["1"][0].view(np.uint32), out["2"][0].view(np.uint32)), "weight gradient bits differ"
    assert np.array_equal(out["1"][1].view(np.uint32), out["2"][1].view(np.uint32)), "bias gradient bits differ"


@pytest.mark.parametrize("N,H,W,Cin,Cout", [(2, 37, 41, 64, 64), (1, 150, 140, 64, 64), (3, 21, 37, 72, 56), (1, 12, 140, 200, 64), (2, 34, 34, 128, 40)])
def test_pingpong_wgrad_64(N, H, W, Cin, Cout, monkeypatch):
    """igemm_wgp64 (64 gradient channels: the taps dealt over the two wave groups) against igemm_wgrad's 64x64 shape: another
    summation order of the same products -- equal to fp32 rounding, bias sums included -- and against the oracle"""
    rng = np.random.RandomState(Cin + Cout + H)
    Ho, Wo = H - 2, W - 2
    x, dz = hu.q(_rand(rng, N, H, W, Cin)), hu.q(_rand(rng, N, Ho, Wo, Cout, scale=0.1))
    xd, dzd = hu.dev_bf16(x), hu.dev_bf16(dz)
    nws = lib().rsu_conv2d_bwd_weight_ws_floats(Cin, Cin, Cout)
    out = {}
    for v in ("0", "1"):
        monkeypatch.setenv("RSU_WG64", v)
        dw = torch.full((3, 3, Cin, Cout), float("nan"), dtype=torch.float32, device=hu.DEV)
        db = torch.full((Cout,), float("nan"), dtype=torch.float32, device=hu.DEV)
        ws = torch.zeros(nws + 1024, dtype=torch.float32, device=hu.DEV)
        ws[nws:] = 777.0
        s = hu.src_of(xd, H, W)
        call("rsu_conv2d_bwd_weight", ctypes.byref(s), hu.ptr(dzd), hu.ptr(dw), hu.ptr(db), hu.ptr(ws), N, Ho, Wo, Cin, 0, Cout, 1, 0, hu.stream())
        assert bool((ws[nws:] == 777.0).all()), "workspace overrun"
        out[v] = (hu.host(dw), hu.host(db))
    ref_dw, ref_db = U.conv2d_bwd_weight(x, dz, dil=1)
    hu.assert_f32_close(out["1"][0], ref_dw, "igemm_wgp64 dW")
    hu.assert_f32_close(out["1"][1], ref_db, "igemm_wgp64 db")
    scale = float(np.abs(out["0"][0]).max())
    assert float(np.abs(out["0"][0] - out["1"][0]).max()) <= 2e-6 * scale + 1e-7
    assert float(np.abs(out["0"][1] - out["1"][1]).max()) <= 2e-6 * float(np.abs(out["0"][1]).max()) + 1e-7


def test_conv2d_bwd_weight_cropped_sources():
    rng = np.random.RandomState(10)
    N, h = 2, 24
    a, c = hu.q(_rand(rng, N, 36, 36, 32)), hu.q(_rand(rng, N, h, h, 64))
    dz = hu.q(_rand(rng, N, h - 2, h - 2, 64, scale=0.1))
    ad, cd, dzd = hu.dev_bf16(a), hu.dev_bf16(c), hu.dev_bf16(dz)
    dw = torch.zeros((3, 3, 96, 64), dtype=torch.float32, device=hu.DEV)
    ws = torch.zeros(lib().rsu_conv2d_bwd_weight_ws_floats(96, 32, 64), dtype=torch.float32, device=hu.DEV)
    for t, off in [(ad, 0), (cd, 32)]:
        s = hu.src_of(t, h, h)
        call("rsu_conv2d_bwd_weight", ctypes.byref(s), hu.ptr(dzd), hu.ptr(dw), None, hu.ptr(ws), N, h - 2, h - 2, 96, off, 64, 1, 0, hu.stream())
    cat = np.concatenate([U.center_crop(a, h, h), c], axis=3)
    hu.assert_f32_close(hu.host(dw), U.conv2d_bwd_weight(cat, dz)[0], "bwd_weight 2 cropped sources")


@pytest.mark.parametrize("ncu", [0, 64])
def test_wgrad_group_equals_single_launches(ncu):
    """rsu_wgrad_group_plan / _run: several layers' weight gradients in ONE launch (every kernel family: the 128x64 ping-pong shape at
    two strip widths, the 64-channel ping-pong shape, a dilated conv and a concat source on the generic kernel, a transposed conv)
    against the oracle and against the single launches (equal up to the summation order of the pixel splits)"""
    from road_segmentation_unet_amd._lib import RsuWgradJob
    rng = np.random.RandomState(77 + ncu)
    N = 2
    # (kind, H, W, Cin_total, ci_off, src C, Cout, dil)
    specs = [(0, 38, 38, 128, 0, 128, 128, 1), (0, 70, 52, 64, 0, 64, 64, 1), (0, 20, 20, 256, 0, 256, 512, 1), (0, 44, 44, 64, 0, 64, 128, 2),
             (0, 30, 30, 96, 32, 64, 192, 1), (1, 11, 13, 128, 0, 128, 64, 1), (0, 150, 26, 128, 0, 128, 128, 1), (0, 33, 47, 64, 0, 64, 64, 2)]
    jobs, keep, checks = [], [], []
    for kind, H, W, cin_t, off, csrc, cout, dil in specs:
        if kind == 0:
            Ho, Wo = H - 2 * dil, W - 2 * dil
            x = hu.q(_rand(rng, N, H, W, csrc))
            dz = hu.q(_rand(rng, N, Ho, Wo, cout, scale=0.1))
            xd, dzd = hu.dev_bf16(x), hu.dev_bf16(dz)
            dw = torch.zeros((3, 3, cin_t, cout), dtype=torch.float32, device=hu.DEV)
            db = torch.full((cout,), float("nan"), dtype=torch.float32, device=hu.DEV)
            jobs.append(RsuWgradJob(0, hu.src_of(xd, H, W), dzd.data_ptr(), dw.data_ptr(), db.data_ptr(), Ho, Wo, cin_t, off, cout, dil))
            rdw, rdb = U.conv2d_bwd_weight(x, dz, dil=dil)
            checks.append((dw, db, rdw, rdb, off, csrc, ("conv", xd, dzd, H, W, Ho, Wo, cin_t, off, cout, dil)))
            keep += [xd, dzd, dw, db]
        else:
            x = hu.q(_rand(rng, N, H, W, cin_t))
            dy = hu.q(_rand(rng, N, 2 * H, 2 * W, cout, scale=0.1))
            K = _rand(rng, 2, 2, cout, cin_t, scale=0.1)
            xd, dyd = hu.dev_bf16(x), hu.dev_bf16(dy)
            dK = torch.full((2, 2, cout, cin_t), float("nan"), dtype=torch.float32, device=hu.DEV)
            db = torch.full((cout,), float("nan"), dtype=torch.float32, device=hu.DEV)
            jobs.append(RsuWgradJob(1, RsuSrc(xd.data_ptr(), H, W, cin_t, 0, 0), dyd.data_ptr(), dK.data_ptr(), db.data_ptr(), 0, 0, 0, 0, cout, 1))
            _, rdK, rdb = U.convT_bwd(x, K, dy, need_dx=False)
            checks.append((dK, db, rdK, rdb, None, None, ("convT", xd, dyd, H, W, cin_t, cout)))
            keep += [xd, dyd, dK, db]
    nws = lib().rsu_wgrad_group_ws_floats()
    ws = torch.zeros(nws + 4096, dtype=torch.float32, device=hu.DEV)
    ws[nws:] = 12345.0
    nb = lib().rsu_wgrad_group_table_bytes()
    host = ctypes.create_string_buffer(nb)
    arr = (RsuWgradJob * len(jobs))(*jobs)
    assert lib().rsu_wgrad_group_plan(arr, len(jobs), hu.ptr(ws), N, ncu, host) == 0
    devt = torch.frombuffer(bytearray(host.raw), dtype=torch.uint8).to(hu.DEV)
    for rep in range(2):   # a second run gives the same bits (fixed summation order)
        call("rsu_wgrad_group_run", host, hu.ptr(devt), hu.stream())
        got = [(hu.host(dw).copy(), hu.host(db).copy()) for dw, db, *_ in checks]
        if rep == 0:
            first = got
        else:
            for (a, b), (c, d) in zip(first, got):
                np.testing.assert_array_equal(a, c)
                np.testing.assert_array_equal(b, d)
    assert bool((ws[nws:] == 12345.0).all()), "workspace overrun"
    ws1 = torch.zeros(max(lib().rsu_conv2d_bwd_weight_ws_floats(256, 256, 512), lib().rsu_convT2x2_bwd_weight_ws_floats(128, 64)) + 64,
                      dtype=torch.float32, device=hu.DEV)
    for (gdw, gdb), (dw, db, rdw, rdb, off, csrc, single) in zip(first, checks):
        if single[0] == "conv":
            hu.assert_f32_close(gdw[:, :, off:off + csrc], rdw, "group conv wgrad")
            assert not gdw[:, :, :off].any() and not gdw[:, :, off + csrc:].any(), "rows outside the source were written"
            hu.assert_f32_close(gdb, rdb, "group conv bias grad")
            _, xd, dzd, H, W, Ho, Wo, cin_t, off_, cout, dil = single
            dw1 = torch.zeros_like(dw)
            db1 = torch.zeros_like(db)
            s = hu.src_of(xd, H, W)
            call("rsu_conv2d_bwd_weight", ctypes.byref(s), hu.ptr(dzd), hu.ptr(dw1), hu.ptr(db1), hu.ptr(ws1), N, Ho, Wo, cin_t, off_, cout, dil, 0, hu.stream())
            scale = float(np.abs(rdw).max())
            assert float(np.abs(hu.host(dw1) - gdw).max()) <= 2e-5 * scale
        else:
            hu.assert_f32_close(gdw, rdw, "group convT wgrad")
            hu.assert_f32_close(gdb, rdb, "group convT bias grad")


@pytest.mark.parametrize("N,H,W,Cin,Cout", [(2, 70, 70, 64, 64), (1, 138, 138, 64, 128), (2, 34, 50, 128, 256), (1, 66, 66, 32, 64),
                                            (1, 282, 150, 64, 64), (3, 22, 22, 64, 192)])
def test_conv2d_fwd_pool_equals_conv_then_pool(N, H, W, Cin, Cout, monkeypatch):
    """rsu_conv2d_fwd_pool (the 2x2 max-pool and its code bytes folded into the conv epilogue: lane swaps on the packed results) against
    rsu_conv2d_fwd followed by rsu_maxpool2x2_fwd_code: activation, pooled tensor and code bytes bit for bit, partial tiles at the image
    edges included; with dropout (keep < 1) and with RSU_POOL_FUSED=0 the call issues the two launches itself: same bits again"""
    rng = np.random.RandomState(N * 7 + H + Cout)
    x = hu.q(_rand(rng, N, H, W, Cin))
    w = _rand(rng, 3, 3, Cin, Cout, scale=1.0 / np.sqrt(9 * Cin))
    b = _rand(rng, Cout, scale=0.1)
    xd, wp, bd = hu.dev_bf16(x), hu.pack_conv_fwd(w), hu.dev_f32(b)
    Ho, Wo = H - 2, W - 2
    s = (RsuSrc * 1)(hu.src_of(xd, H, W))

    def run(fused, keep=1.0, key=0):
        y = torch.full((N, Ho, Wo, Cout), float("nan"), dtype=torch.bfloat16, device=hu.DEV)
        pool = torch.full((N, Ho // 2, Wo // 2, Cout), float("nan"), dtype=torch.bfloat16, device=hu.DEV)
        code = torch.full((N, Ho // 2, Wo // 2, Cout), 0xAA, dtype=torch.uint8, device=hu.DEV)
        if fused:
            call("rsu_conv2d_fwd_pool", s, 1, hu.ptr(wp), hu.ptr(bd), hu.ptr(y), hu.ptr(pool), hu.ptr(code), N, H, W, Cout, keep, key, 0, hu.stream())
        else:
            call("rsu_conv2d_fwd", s, 1, hu.ptr(wp), hu.ptr(bd), hu.ptr(y), N, H, W, Cout, 1, 1, 0, hu.stream())
            call("rsu_maxpool2x2_fwd_code", hu.ptr(y), hu.ptr(pool), hu.ptr(code), N, Ho, Wo, Cout, keep, key, hu.stream())
        torch.cuda.synchronize()
        return y.view(torch.int16).cpu().numpy(), pool.view(torch.int16).cpu().numpy(), code.cpu().numpy()

    ref = run(False)
    monkeypatch.setenv("RSU_POOL_FUSED", "2")   # fold wherever a tile shape can (the default folds only where it costs the conv no extra round)
    got = run(True)
    for a, r, what in zip(got, ref, ("activation", "pooled", "code bytes")):
        np.testing.assert_array_equal(a, r, err_msg=what)
    assert float((ref[1] != 0).mean()) > 0.3
    ref_d, got_d = run(False, 0.8, 1234), run(True, 0.8, 1234)
    for a, r in zip(got_d, ref_d):
        np.testing.assert_array_equal(a, r)
    for mode in ("0", "1"):
        monkeypatch.setenv("RSU_POOL_FUSED", mode)
        for a, r in zip(run(True), ref):
            np.testing.assert_array_equal(a, r)


# ------------------------------------------------------------------------------------------- first layer
@pytest.mark.parametrize("dil,keep", [(1, 1.0), (2, 1.0), (1, 0.8)])
def test_color_adjust_and_first_conv(dil, keep):
    rng = np.random.RandomState(11 + dil)
    key = 0xC0FFEE11
    N, H, W, Cout = 2, 29, 35, 64
    x = rng.rand(N, H, W, 3).astype(np.float32)
    w0 = _rand(rng, 3, 3, scale=0.5)
    b0 = _rand(rng, 3, scale=0.1)
    w1 = _rand(rng, 3, 3, 3, Cout, scale=0.3)
    b1 = _rand(rng, Cout, scale=0.1)
    in16 = torch.zeros((N, H, W, 16), dtype=torch.bfloat16, device=hu.DEV)
    xd_, w0d, b0d, w1d, b1d = hu.dev_f32(x), hu.dev_f32(w0), hu.dev_f32(b0), hu.dev_f32(w1), hu.dev_f32(b1)  # keep alive
    call("rsu_color_adjust_fwd", hu.ptr(xd_), hu.ptr(w0d), hu.ptr(b0d), hu.ptr(in16), N * H * W, keep, key, hu.stream())
    got16 = hu.host(in16)
    m = U.dropout_mask((N, H, W, 3), keep, key) if keep < 1.0 else np.ones((N, H, W, 3), np.float32)
    if keep < 1.0:
        assert 0.7 < m.mean() < 0.9
    net0 = U.conv1x1_fwd(x, w0, b0, sub=0.5) * m * (np.float32(1) / np.float32(keep))
    hu.assert_bf16_close(got16[..., 0:3], net0, "color_adjust net0 (dropout keep=%g)" % keep)
    for ci in range(3):
        for cj in range(3):
            hu.assert_bf16_close(got16[..., 4 + 3 * ci + cj], (x[..., ci] - 0.5) * m[..., cj], "color_adjust xc*m")
    np.testing.assert_array_equal(got16[..., 13:16], m)
    assert not got16[..., 3].any()
    Ho, Wo = H - 2 * dil, W - 2 * dil
    y = torch.full((N, Ho, Wo, Cout), float("nan"), dtype=torch.bfloat16, device=hu.DEV)
    pk1 = torch.zeros(lib().rsu_packed_first_bytes(Cout) // 2, dtype=torch.bfloat16, device=hu.DEV)
    call("rsu_pack_conv_first", hu.ptr(w1d), hu.ptr(pk1), Cout, hu.stream())
    call("rsu_conv_first_fwd", hu.ptr(in16), hu.ptr(pk1), hu.ptr(b1d), hu.ptr(y), N, H, W, Cout, dil, 0, hu.stream())
    ref = U.conv2d_fwd(got16[..., 0:3], hu.q(w1), b1, dil=dil)
    hu.assert_bf16_close(hu.host(y), ref, "conv_first_fwd")
    # weight gradients (MFMA narrow wgrad over the 16-channel tensor)
    dz = hu.q(_rand(rng, N, Ho, Wo, Cout, scale=0.1))
    dw1 = torch.zeros((3, 3, 3, Cout), dtype=torch.float32, device=hu.DEV)
    gx = torch.zeros((9, 12, Cout), dtype=torch.float32, device=hu.DEV)
    ws = torch.zeros(lib().rsu_conv_first_bwd_ws_floats(Cout), dtype=torch.float32, device=hu.DEV)
    dzd = hu.dev_bf16(dz)
    dbf = torch.zeros(Cout, dtype=torch.float32, device=hu.DEV)
    call("rsu_conv_first_bwd_weight", hu.ptr(in16), hu.ptr(dzd), hu.ptr(dw1), hu.ptr(gx), hu.ptr(dbf), hu.ptr(ws), N, H, W, Cout, dil, 0, hu.stream())
    hu.assert_f32_close(hu.host(dbf), dz.reshape(-1, Cout).astype(np.float64).sum(0), "conv_first db")
    hu.assert_f32_close(hu.host(dw1), U.conv2d_bwd_weight(got16[..., 0:3], dz, dil=dil)[0], "conv_first dW")
    ref_gx = U.conv2d_bwd_weight(got16[..., 4:16], dz, dil=dil)[0].reshape(9, 12, Cout)  # rows: 9 masked (x-0.5) products, 3 mask sums
    hu.assert_f32_close(hu.host(gx), ref_gx, "conv_first gx")


@pytest.mark.parametrize("N,H,W,Cout,dil", [(2, 200, 203, 64, 1), (1, 40, 37, 16, 2), (3, 21, 50, 72, 1), (1, 64, 64, 160, 2), (1, 5, 19, 8, 1), (4, 572, 572, 64, 1)])
def test_colour_adjust_fused_into_the_first_conv_gives_the_two_launches_bits(N, H, W, Cout, dil):
    """rsu_color_conv_first_fwd (unet.py:22-23 + 34-35 from the f32 input in one launch: round 6) against
    rsu_color_adjust_fwd(keep = 1) + rsu_conv_first_fwd: bit for bit (NaN-prefilled outputs), and against the oracle -- ragged row ends,
    more pieces than waves, channel counts that are not multiples of 64, both dilations, and the c2 level-0 shape itself"""
    rng = np.random.RandomState(5 + H)
    x = rng.rand(N, H, W, 3).astype(np.float32)
    w0, b0 = _rand(rng, 3, 3, scale=0.5), _rand(rng, 3, scale=0.1)
    w1, b1 = _rand(rng, 3, 3, 3, Cout, scale=0.3), _rand(rng, Cout, scale=0.1)
    xd_, w0d, b0d, w1d, b1d = hu.dev_f32(x), hu.dev_f32(w0), hu.dev_f32(b0), hu.dev_f32(w1), hu.dev_f32(b1)
    in16 = torch.zeros((N, H, W, 16), dtype=torch.bfloat16, device=hu.DEV)
    Ho, Wo = H - 2 * dil, W - 2 * dil
    pk1 = torch.zeros(lib().rsu_packed_first_bytes(Cout) // 2, dtype=torch.bfloat16, device=hu.DEV)
    call("rsu_pack_conv_first", hu.ptr(w1d), hu.ptr(pk1), Cout, hu.stream())
    ya = torch.full((N, Ho, Wo, Cout), float("nan"), dtype=torch.bfloat16, device=hu.DEV)
    yb = torch.full((N, Ho, Wo, Cout), float("nan"), dtype=torch.bfloat16, device=hu.DEV)
    call("rsu_color_adjust_fwd", hu.ptr(xd_), hu.ptr(w0d), hu.ptr(b0d), hu.ptr(in16), N * H * W, 1.0, 0, hu.stream())
    call("rsu_conv_first_fwd", hu.ptr(in16), hu.ptr(pk1), hu.ptr(b1d), hu.ptr(ya), N, H, W, Cout, dil, 0, hu.stream())
    call("rsu_color_conv_first_fwd", hu.ptr(xd_), hu.ptr(w0d), hu.ptr(b0d), hu.ptr(pk1), hu.ptr(b1d), hu.ptr(yb), N, H, W, Cout, dil, 0, hu.stream())
    torch.cuda.synchronize()
    assert not bool(torch.isnan(yb.float()).any())
    assert torch.equal(ya.view(torch.int16), yb.view(torch.int16))
    if H <= 203:   # (the oracle's conv on the device's own bf16 net0, as in test_color_adjust_and_first_conv: a 1-ulp flip of net0 is not this kernel's)
        hu.assert_bf16_close(hu.host(yb), U.conv2d_fwd(hu.host(in16)[..., 0:3], hu.q(w1), b1, dil=dil), "colour adjust + first conv, one launch")


@pytest.mark.parametrize("N,H,W,Cout,dil", [(2, 200, 203, 64, 1), (1, 40, 37, 16, 2), (3, 21, 50, 72, 1), (1, 64, 64, 160, 2), (1, 5, 19, 8, 1)])
def test_first_conv_kernel_against_oracle_and_generic_launch(N, H, W, Cout, dil, monkeypatch):
    """k_conv_first_fwd (weights in registers, pixels straight from global memory; the default of rsu_conv_first_fwd) against the oracle and
    against the same layer as a launch of the generic implicit-GEMM kernels (RSU_FIRST_GEN=0): more pieces than waves, ragged row ends,
    channel counts that are not multiples of 64, both dilations. The two kernels sum the 9 x 16 products in another order: equal
    to one bf16 rounding step."""
    rng = np.random.RandomState(H + Cout)
    in16 = hu.q(_rand(rng, N, H, W, 16))
    w1 = _rand(rng, 3, 3, 3, Cout, scale=0.3)
    b1 = _rand(rng, Cout, scale=0.1)
    ind, w1d, b1d = hu.dev_bf16(in16), hu.dev_f32(w1), hu.dev_f32(b1)
    pk1 = torch.zeros(lib().rsu_packed_first_bytes(Cout) // 2, dtype=torch.bfloat16, device=hu.DEV)
    call("rsu_pack_conv_first", hu.ptr(w1d), hu.ptr(pk1), Cout, hu.stream())
    Ho, Wo = H - 2 * dil, W - 2 * dil
    out = {}
    for gen in ("1", "0"):
        monkeypatch.setenv("RSU_FIRST_GEN", gen)
        y = torch.full((N, Ho, Wo, Cout), float("nan"), dtype=torch.bfloat16, device=hu.DEV)
        call("rsu_conv_first_fwd", hu.ptr(ind), hu.ptr(pk1), hu.ptr(b1d), hu.ptr(y), N, H, W, Cout, dil, 0, hu.stream())
        out[gen] = hu.host(y)
        hu.assert_bf16_close(out[gen], U.conv2d_fwd(in16[..., 0:3], hu.q(w1), b1, dil=dil), "conv_first_fwd gen " + gen)
    d = np.abs(out["1"].astype(np.float64) - out["0"].astype(np.float64))
    assert d.max() <= 2.0 ** -7 * max(1.0, np.abs(out["0"]).max()), d.max()
    assert (d > 0).mean() < 0.01


@pytest.mark.parametrize("N,H,W,Cout,dil", [(2, 200, 203, 64, 1), (1, 40, 37, 16, 2), (3, 21, 50, 72, 1), (1, 64, 64, 160, 2), (1, 5, 19, 8, 1),
                                            (4, 130, 126, 64, 1)])
@pytest.mark.parametrize("ncu", [0, 128, 32])
def test_first_conv_weight_gradient_pingpong_against_generic_launch(N, H, W, Cout, dil, ncu, monkeypatch):
    """igemm_wg1 (default of rsu_conv_first_bwd_weight: nine phase images of in16, every wave holds the whole 64 x 16 x 9 block, the
    groups alternate tiles) against the generic 64x16 igemm_wgrad launch (RSU_WG1_GEN=1) and the oracle: one tile per workgroup and
    dozens (CU budget 32), pixel counts that are not multiples of 128, channel blocks that are not full, both dilations. Another
    summation order: equal to fp32 noise; repeatable bit for bit."""
    rng = np.random.RandomState(H + Cout)
    in16 = hu.q(_rand(rng, N, H, W, 16))
    Ho, Wo = H - 2 * dil, W - 2 * dil
    dz = hu.q(_rand(rng, N, Ho, Wo, Cout, scale=0.1))
    ind, dzd = hu.dev_bf16(in16), hu.dev_bf16(dz)
    ws = torch.zeros(lib().rsu_conv_first_bwd_ws_floats(Cout), dtype=torch.float32, device=hu.DEV)
    out = {}
    for gen in ("2", "1", "2"):
        monkeypatch.setenv("RSU_WG1_GEN", gen)
        dw1 = torch.full((3, 3, 3, Cout), float("nan"), dtype=torch.float32, device=hu.DEV)
        gx = torch.full((9, 12, Cout), float("nan"), dtype=torch.float32, device=hu.DEV)
        db = torch.full((Cout,), float("nan"), dtype=torch.float32, device=hu.DEV)
        ws.fill_(float("nan"))
        call("rsu_conv_first_bwd_weight", hu.ptr(ind), hu.ptr(dzd), hu.ptr(dw1), hu.ptr(gx), hu.ptr(db), hu.ptr(ws), N, H, W, Cout, dil, ncu, hu.stream())
        if gen in out:
            for a, b in zip((dw1, gx, db), out[gen]):
                assert torch.equal(a, b), "the ping-pong kernel must repeat bit for bit"
        out[gen] = (dw1, gx, db)
    hu.assert_f32_close(hu.host(out["2"][2]), dz.reshape(-1, Cout).astype(np.float64).sum(0), "conv_first db (ping-pong)")
    hu.assert_f32_close(hu.host(out["2"][0]), U.conv2d_bwd_weight(in16[..., 0:3], dz, dil=dil)[0], "conv_first dW (ping-pong)")
    hu.assert_f32_close(hu.host(out["2"][1]), U.conv2d_bwd_weight(in16[..., 4:16], dz, dil=dil)[0].reshape(9, 12, Cout), "conv_first gx (ping-pong)")
    for a, b in zip(out["2"], out["1"]):
        a, b = hu.host(a).astype(np.float64), hu.host(b).astype(np.float64)
        assert np.abs(a - b).max() <= 2e-5 * max(1.0, np.abs(b).max()), np.abs(a - b).max()


# ------------------------------------------------------------------------------------------- pool
@pytest.mark.parametrize("Cout,scale", [(64, 1.0), (16, 1.25), (72, 1.0)])
def test_color_adjust_bwd_from_scatter_buffer(Cout, scale):
    """rsu_color_adjust_bwd against the two sums of include/rsu.h in float64 (the formula itself is pinned against the oracle's
    color_space_adjust gradients by test_color_adjust_and_first_conv and the whole-net gradient tests)."""
    rng = np.random.RandomState(Cout)
    gx = rng.randn(9, 12, Cout).astype(np.float32)
    w1 = rng.randn(3, 3, 3, Cout).astype(np.float32)
    w9 = w1.reshape(9, 3, Cout).astype(np.float64)
    dW = np.einsum("tjo,tijo->ij", w9, gx[:, :9].reshape(9, 3, 3, Cout).astype(np.float64)) * scale
    db = np.einsum("tjo,tjo->j", w9, gx[:, 9:].astype(np.float64)) * scale
    dWd, dbd = torch.full((3, 3), 7.0, device=hu.DEV), torch.full((3,), 7.0, device=hu.DEV)
    gxd, w1d = hu.dev_f32(gx), hu.dev_f32(w1)
    call("rsu_color_adjust_bwd", hu.ptr(gxd), hu.ptr(w1d), hu.ptr(dWd), hu.ptr(dbd), Cout, scale, 0, hu.stream())
    np.testing.assert_allclose(hu.host(dWd), dW, rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(hu.host(dbd), db, rtol=2e-5, atol=2e-5)
    call("rsu_color_adjust_bwd", hu.ptr(gxd), hu.ptr(w1d), hu.ptr(dWd), hu.ptr(dbd), Cout, scale, 1, hu.stream())  # accumulate
    np.testing.assert_allclose(hu.host(dWd), 2 * dW, rtol=2e-5, atol=4e-5)
    np.testing.assert_allclose(hu.host(dbd), 2 * db, rtol=2e-5, atol=4e-5)


@pytest.mark.parametrize("N,H,W,C", [(2, 12, 16, 64), (1, 30, 26, 16), (1, 9, 11, 8)])
def test_maxpool_fwd_and_junction_bwd(N, H, W, C):
    rng = np.random.RandomState(H + C)
    x = hu.q(np.maximum(_rand(rng, N, H, W, C), 0))
    x[0, :4, :4, :] = x[0, 0, 0, :]  # force ties (incl. zeros) in a corner
    xd = hu.dev_bf16(x)
    y = torch.zeros((N, H // 2, W // 2, C), dtype=torch.bfloat16, device=hu.DEV)
    call("rsu_maxpool2x2_fwd", hu.ptr(xd), hu.ptr(y), N, H, W, C, 1.0, 0, hu.stream())
    np.testing.assert_array_equal(hu.host(y), U.maxpool_fwd(x))
    # with the next level's dropout fused (unet.py:29-30)
    keep, key = 0.8, 0x1234ABCD
    mk = U.dropout_mask(y.shape, keep, key) * (np.float32(1) / np.float32(keep))
    call("rsu_maxpool2x2_fwd", hu.ptr(xd), hu.ptr(y), N, H, W, C, keep, key, hu.stream())
    np.testing.assert_array_equal(hu.host(y), hu.q(U.maxpool_fwd(x) * mk))
    Hs, Ws = H - 4, W - 6
    dpool = hu.q(_rand(rng, N, H // 2, W // 2, C))
    dskip = hu.q(_rand(rng, N, Hs, Ws, C))
    dpd, dsd = hu.dev_bf16(dpool), hu.dev_bf16(dskip)
    for use_pool, use_skip, kp in [(1, 1, 1.0), (1, 0, 1.0), (0, 1, 1.0), (1, 1, keep)]:
        dz = torch.full((N, H, W, C), float("nan"), dtype=torch.bfloat16, device=hu.DEV)
        call("rsu_pool_skip_relu_bwd", hu.ptr(xd), hu.ptr(dpd) if use_pool else None,
             hu.ptr(dsd) if use_skip else None, hu.ptr(dz), N, H, W, C, Hs, Ws, kp, key, hu.stream())
        g = np.zeros_like(x)
        if use_pool:
            xe = x[:, :H // 2 * 2, :W // 2 * 2]
            g[:, :H // 2 * 2, :W // 2 * 2] += U.maxpool_bwd(xe, dpool * mk if kp < 1.0 else dpool)
        if use_skip:
            g += U.center_pad_like(dskip, x.shape)
        ref = U.relu_bwd(x, g)
        hu.assert_bf16_close(hu.host(dz), ref, "pool_skip_relu_bwd pool=%d skip=%d" % (use_pool, use_skip))
        if H % 2 == 0 and W % 2 == 0:
            # the same junction from the pool's code bytes (argmax + ReLU bits) instead of the activation: the same bits
            code = torch.full((N, H // 2, W // 2, C), 255, dtype=torch.uint8, device=hu.DEV)
            y2 = torch.zeros_like(y)
            call("rsu_maxpool2x2_fwd_code", hu.ptr(xd), hu.ptr(y2), hu.ptr(code), N, H, W, C, kp, key, hu.stream())
            dz2 = torch.full((N, H, W, C), float("nan"), dtype=torch.bfloat16, device=hu.DEV)
            call("rsu_pool_skip_relu_bwd_code", None, hu.ptr(code), hu.ptr(dpd) if use_pool else None,
                 hu.ptr(dsd) if use_skip else None, hu.ptr(dz2), N, H, W, C, Hs, Ws, kp, key, hu.stream())
            assert torch.equal(dz.view(torch.int16), dz2.view(torch.int16)), "code-byte junction differs"


# ------------------------------------------------------------------------------------------- transposed conv
@pytest.mark.parametrize("N,H,W,Cin,Cout", [(2, 7, 9, 128, 64), (1, 14, 14, 64, 32), (1, 26, 24, 32, 16), (1, 28, 28, 256, 128),
                                            (4, 28, 28, 1024, 512), (2, 52, 50, 96, 96), (1, 20, 21, 96, 160), (3, 33, 31, 72, 64)])
def test_convT(N, H, W, Cin, Cout):
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
    xd = hu.dev_bf16(x)
    y = torch.full((N, 2 * H, 2 * W, Cout), float("nan"), dtype=torch.bfloat16, device=hu.DEV)
    bd = hu.dev_f32(b)
    call("rsu_convT2x2_fwd", hu.ptr(xd), hu.ptr(pf), hu.ptr(bd), hu.ptr(y), N, H, W, Cin, Cout, 0, hu.stream())
    hu.assert_bf16_close(hu.host(y), U.convT_fwd(x, hu.q(K), b), "convT fwd")
    dy = hu.q(_rand(rng, N, 2 * H, 2 * W, Cout, scale=0.1))
    dyd = hu.dev_bf16(dy)
    dx = torch.full((N, H, W, Cin), float("nan"), dtype=torch.bfloat16, device=hu.DEV)
    call("rsu_convT2x2_bwd_data", hu.ptr(dyd), hu.ptr(pb), hu.ptr(dx), hu.ptr(xd), 1.0, N, H, W, Cin, Cout, 0, hu.stream())
    rdx, rdK, rdb = U.convT_bwd(x, hu.q(K), dy)
    hu.assert_bf16_close(hu.host(dx), U.relu_bwd(x, rdx), "convT bwd_data")
    # dropout in front of the transposed conv (unet.py:64-65): forward kernel + backward fused as (mask source, scale)
    keep, key = 0.8, 0x5EED0001
    inv = np.float32(1) / np.float32(keep)
    xdrop = torch.full((N, H, W, Cin), float("nan"), dtype=torch.bfloat16, device=hu.DEV)
    call("rsu_dropout_fwd", hu.ptr(xd), hu.ptr(xdrop), x.size, keep, key, hu.stream())
    m = U.dropout_mask(x.shape, keep, key)
    np.testing.assert_array_equal(hu.host(xdrop), hu.q(x * m * inv))
    call("rsu_convT2x2_bwd_data", hu.ptr(dyd), hu.ptr(pb), hu.ptr(dx), hu.ptr(xdrop), float(inv), N, H, W, Cin, Cout, 0, hu.stream())
    hu.assert_bf16_close(hu.host(dx), U.relu_bwd(x, rdx * m * inv), "convT bwd_data with dropout")
    dK = torch.full((2, 2, Cout, Cin), float("nan"), dtype=torch.float32, device=hu.DEV)
    nws = lib().rsu_convT2x2_bwd_weight_ws_floats(Cin, Cout)
    ws = torch.zeros(nws + 4096, dtype=torch.float32, device=hu.DEV)
    ws[nws:] = 12345.0  # guard band: at 64 < Cin < 128 igemm_wgt splits the pixels further than the generic kernel the workspace was once sized for
    dbT = torch.full((Cout,), float("nan"), dtype=torch.float32, device=hu.DEV)
    call("rsu_convT2x2_bwd_weight", hu.ptr(xd), hu.ptr(dyd), hu.ptr(dK), hu.ptr(dbT), hu.ptr(ws), N, H, W, Cin, Cout, 0, hu.stream())
    assert bool((ws[nws:] == 12345.0).all()), "workspace overrun"
    hu.assert_f32_close(hu.host(dK), rdK, "convT bwd_weight")
    hu.assert_f32_close(hu.host(dbT), rdb, "convT bias grad fused in bwd_weight")


@pytest.mark.parametrize("N,H,W,Cin,Cout", [(4, 100, 100, 256, 128), (1, 7, 9, 128, 64), (2, 33, 31, 72, 96), (3, 28, 28, 1024, 512), (1, 61, 67, 64, 32),
                                            (2, 50, 52, 200, 160)])
@pytest.mark.parametrize("ncu", [0, 128, 64])
def test_convT_weight_gradient_pingpong_against_generic_launch(N, H, W, Cin, Cout, ncu, monkeypatch):
    """igemm_wgt (RSU_WGT_GEN=3: phase images of dy, ping-pong over the k-steps, flat 64-pixel tiles) against the generic 4-tap stride-2
    igemm_wgrad launch (RSU_WGT_GEN=1) and the oracle: many tiles per workgroup, a single tile (one split: written in place), pixel
    counts that are not multiples of 64, channel blocks that are not full, every CU budget the schedules use. The two kernels sum the
    pixels in another order: equal to fp32 summation noise; each is repeatable bit for bit."""
    rng = np.random.RandomState(H + Cin)
    x = hu.q(np.maximum(_rand(rng, N, H, W, Cin), 0))
    dy = hu.q(_rand(rng, N, 2 * H, 2 * W, Cout, scale=0.1))
    xd, dyd = hu.dev_bf16(x), hu.dev_bf16(dy)
    ws = torch.zeros(lib().rsu_convT2x2_bwd_weight_ws_floats(Cin, Cout), dtype=torch.float32, device=hu.DEV)
    out = {}
    for gen in ("3", "1", "3"):
        monkeypatch.setenv("RSU_WGT_GEN", gen)
        dK = torch.full((2, 2, Cout, Cin), float("nan"), dtype=torch.float32, device=hu.DEV)
        db = torch.full((Cout,), float("nan"), dtype=torch.float32, device=hu.DEV)
        ws.fill_(float("nan"))
        call("rsu_convT2x2_bwd_weight", hu.ptr(xd), hu.ptr(dyd), hu.ptr(dK), hu.ptr(db), hu.ptr(ws), N, H, W, Cin, Cout, ncu, hu.stream())
        if gen in out:
            assert torch.equal(dK, out[gen][0]) and torch.equal(db, out[gen][1]), "the ping-pong kernel must repeat bit for bit"
        out[gen] = (dK, db)
    if N * H * W * Cin * Cout <= 3e9:   # (the oracle's loops: seconds)
        rdK, rdb = U.convT_bwd(x, np.zeros((2, 2, Cout, Cin), np.float32), dy)[1:]
        hu.assert_f32_close(hu.host(out["3"][0]), rdK, "convT bwd_weight (ping-pong)")
        hu.assert_f32_close(hu.host(out["3"][1]), rdb, "convT bias grad (ping-pong)")
    for a, b in zip(out["3"], out["1"]):
        a, b = hu.host(a).astype(np.float64), hu.host(b).astype(np.float64)
        assert np.abs(a - b).max() <= 2e-5 * max(1.0, np.abs(b).max()), np.abs(a - b).max()


# ------------------------------------------------------------------------------------------- head, optimizer
@pytest.mark.parametrize("C", [64, 16])
def test_head(C):
    rng = np.random.RandomState(C)
    npix = 3 * 37 * 41
    act = hu.q(np.maximum(_rand(rng, npix, C), 0))
    w = _rand(rng, C, 2, scale=0.3)
    b = _rand(rng, 2, scale=0.1)
    labels = (rng.rand(npix) < 0.2).astype(np.int64)
    ad, wd, bd = hu.dev_bf16(act), hu.dev_f32(w), hu.dev_f32(b)
    prob = torch.zeros(npix, dtype=torch.float32, device=hu.DEV)
    logits = torch.zeros((npix, 2), dtype=torch.float32, device=hu.DEV)
    call("rsu_head_fwd", hu.ptr(ad), hu.ptr(wd), hu.ptr(bd), hu.ptr(prob), hu.ptr(logits), npix, C, hu.stream())
    ref_logits = U.conv1x1_fwd(act, w, b)
    rp, rloss, rdl = U.softmax_ce(ref_logits, labels)
    hu.assert_f32_close(hu.host(logits), ref_logits, "head logits", rtol=1e-5)
    hu.assert_f32_close(hu.host(prob), rp, "head prob", rtol=1e-4, atol_scale=1e-6)
    inv = 1.0 / (2 * npix)  # as if this rank held half of the global batch
    dact = torch.zeros((npix, C), dtype=torch.bfloat16, device=hu.DEV)
    dw = torch.zeros((C, 2), dtype=torch.float32, device=hu.DEV)
    db = torch.zeros(2, dtype=torch.float32, device=hu.DEV)
    loss = torch.zeros(1, dtype=torch.float32, device=hu.DEV)
    ws = torch.zeros(lib().rsu_head_ws_floats(npix, C), dtype=torch.float32, device=hu.DEV)
    lab = torch.from_numpy(labels).to(hu.DEV)
    call("rsu_head_fwd_bwd", hu.ptr(ad), hu.ptr(wd), hu.ptr(bd), hu.ptr(lab), hu.ptr(prob), hu.ptr(loss), hu.ptr(dact), hu.ptr(dw), hu.ptr(db),
         hu.ptr(ws), npix, C, inv, hu.stream())
    rdl = rdl * 0.5  # oracle's dlogits are /npix; this call scales by 1/(2 npix)
    rdx, rdw, rdb = U.conv1x1_bwd(act, w, rdl)
    assert abs(float(hu.host(loss)[0]) / npix - rloss) < 2e-5 * max(1.0, abs(rloss))
    hu.assert_bf16_close(hu.host(dact), U.relu_bwd(act, rdx), "head dact")
    hu.assert_f32_close(hu.host(dw), rdw, "head dw")
    hu.assert_f32_close(hu.host(db), rdb, "head db")


def test_momentum_step():
    rng = np.random.RandomState(3)
    n = 1003
    w, a, g = _rand(rng, n), _rand(rng, n), _rand(rng, n)
    wd, ad, gd = torch.zeros(1004, device=hu.DEV), torch.zeros(1004, device=hu.DEV), torch.zeros(1004, device=hu.DEV)
    wd[:n], ad[:n], gd[:n] = hu.dev_f32(w), hu.dev_f32(a), hu.dev_f32(g)
    call("rsu_momentum_step", hu.ptr(wd), hu.ptr(ad), hu.ptr(gd), 0.01, 0.9, 1.0, n, hu.stream())
    U.momentum_step(w, a, g, 0.01, 0.9)
    np.testing.assert_allclose(hu.host(ad)[:n], a, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(hu.host(wd)[:n], w, rtol=1e-6, atol=1e-7)
    assert float(hu.host(wd)[n]) == 0.0


# ------------------------------------------------------------------------------------------- tiler
@pytest.mark.parametrize("H,P,S,stride,nimg", [(20, 8, 12, 4, 2), (44, 20, 60, 12, 3), (16, 16, 24, 16, 1)])
def test_tiler_extract_and_overlap(H, P, S, stride, nimg):
    rng = np.random.RandomState(H)
    imgs = rng.rand(nimg, H, H, 3).astype(np.float32)
    pps = (H - P) // stride + 1
    nt = nimg * pps * pps
    tiles = torch.zeros((nt, S, S, 3), dtype=torch.float32, device=hu.DEV)
    idev = hu.dev_f32(imgs)
    half = nt // 2
    if half:
        call("rsu_extract_tiles", hu.ptr(idev), hu.ptr(tiles), nimg, H, S, P, stride, 0, half, hu.stream())
    call("rsu_extract_tiles", hu.ptr(idev), hu.ptr(tiles[half:]), nimg, H, S, P, stride, half, nt - half, hu.stream())
    ref = T.extract_patches(T.mirror_border(imgs, (S - P) // 2), S, stride=stride, predict_patch_size=P)
    np.testing.assert_array_equal(hu.host(tiles), ref.astype(np.float32))  # bit-exact: pure data movement
    prob = rng.rand(nt, P, P).astype(np.float32)
    acc = torch.zeros((nimg, H, H), dtype=torch.float32, device=hu.DEV)
    hits = torch.zeros((nimg, H, H), dtype=torch.float32, device=hu.DEV)
    pdev = hu.dev_f32(prob)
    if half:
        call("rsu_overlap_add", hu.ptr(pdev), hu.ptr(acc), hu.ptr(hits), nimg, H, P, stride, 0, half, hu.stream())
    call("rsu_overlap_add", hu.ptr(pdev[half:]), hu.ptr(acc), hu.ptr(hits), nimg, H, P, stride, half, nt - half, hu.stream())
    out = torch.zeros_like(acc)
    call("rsu_overlap_finish", hu.ptr(acc), hu.ptr(hits), hu.ptr(out), acc.numel(), hu.stream())
    refm = T.images_from_patches(prob.astype(np.float64).reshape(nimg, pps * pps, P, P, 1), stride=stride)[..., 0]
    np.testing.assert_allclose(hu.host(out), refm, rtol=2e-6, atol=1e-7)


def test_abi_rejects_bad_geometry():
    """error behaviour: the reference asserts (unet.py:108, images.py:60-61); the ABI returns RSU_EINVAL"""
    o = ctypes.c_int()
    assert lib().rsu_input_size_needed(128, 5, ctypes.byref(o)) == -22
    assert lib().rsu_extract_tiles(None, None, 1, 20, 12, 8, 5, 0, 1, None) == -22
