"""-m gpu: the persistent conv kernels at the CU shares the schedules hand out, on shapes with many tiles per workgroup.
include/rsu.h: "for every other launch [ncu] only changes speed". The op tests call every MFMA launch with ncu = 0 (the whole chip), where
their shapes give each persistent workgroup one tile; the tile loops (igemm_pp / igemm_pp_d2 / igemm_fwd2: advance() by the tile stride,
the halo prefetch of the next tile; igemm_ct: pf_tile, epi_setup_tile), the workgroup-id remapping of pick_cob_group and the planner's
large tiles at small shares then never run at op level. Here every launch runs at SHARES, ncu passed explicitly (the process default is
never touched): the 256-CU result against the oracle (the op tolerances of hiputil), every other share against the 256-CU result BIT FOR
BIT, and -- from the planner's RSU_PLAN_DEBUG line -- at 32 CUs at least three rounds of tiles with a short last one. The weight gradients,
whose summation order ncu legitimately changes, are checked per share against the oracle and for repeatability."""
import ctypes
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_oracle as U  # noqa: E402
from road_segmentation_unet_amd._lib import RsuSrc, call, lib  # noqa: E402
from tests import hiputil as hu  # noqa: E402
from tests.test_gpu_ops import SPLITK_SHAPES  # noqa: E402

# the whole chip; the shares schedule.cu_shares hands out (128 + 128, 112 + 128, 96 + 128); a small share that is no power of two; the minimum
SHARES = (256, 128, 112, 104, 96, 40, 32)
WGRAD_SHARES = (32, 96, 104, 112, 128)


def _rand(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def _nan(*shape, dtype=torch.bfloat16):
    return torch.full(shape, float("nan"), dtype=dtype, device=hu.DEV)


def _bits(t):
    torch.cuda.synchronize()
    return (t if t.dtype == torch.uint8 else t.view(torch.int16)).cpu().numpy().copy()


def _value(bits):
    """bf16 bit pattern (int16) -> float32"""
    return torch.from_numpy(bits).view(torch.bfloat16).to(torch.float32).numpy()


def _plan_fields(capfd):
    """the last [plan fwd2] line on stderr since the previous read, as {field: int} (tiles, grid, rounds, TN, Cout, ksplit, cgrp, ...)"""
    lines = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[plan fwd2]")]
    assert lines, "no plan line: RSU_PLAN_DEBUG=1 not seen by the launch"
    f = {k: int(v) for k, v in re.findall(r"\b([A-Za-z_]+)(\d+)\b", lines[-1].split("pix_util")[0])}
    f["line"] = lines[-1]
    return f


def _assert_same_bits(ref, got, what, ncu, ref_name="256 CUs"):
    if np.array_equal(ref, got):
        return
    assert ref.shape == got.shape, (what, ref.shape, got.shape)
    diff = ref != got
    idx = tuple(int(i) for i in np.argwhere(diff)[0])
    raise AssertionError("%s: ncu = %s differs from %s in %d/%d elements; first at (n, y, x, c) = %s: %r vs %r"
                         % (what, ncu, ref_name, int(diff.sum()), diff.size, idx, got[idx], ref[idx]))


def _assert_tile_loop_ran(f, what):
    """condition (c) on the INPUTS of a case: at 32 CUs a workgroup walks at least three tiles and the last round is short"""
    ncob = -(-f["Cout"] // f["TN"])
    workers = f["grid"] // (ncob * f["ksplit"])
    assert f["rounds"] >= 3 and f["tiles"] % workers != 0, "%s: the shape is too small for the tile loop at 32 CUs: %s" % (what, f["line"])


def _across_shares(capfd, what, launch, shares=SHARES, plan=True):
    """launch(ncu) -> tuple of freshly pre-filled device tensors. Every share must reproduce the bits of the first one (256 CUs).
    Returns (bits at 256 CUs, {ncu: plan fields})."""
    ref, plans = None, {}
    for ncu in shares:
        capfd.readouterr()
        bits = tuple(_bits(t) for t in launch(ncu))
        if plan:
            plans[ncu] = _plan_fields(capfd)
        if ref is None:
            ref = bits
        else:
            for i, (r, g) in enumerate(zip(ref, bits)):
                _assert_same_bits(r, g, "%s output %d" % (what, i), ncu)
    for i, r in enumerate(ref):
        if r.dtype == np.int16:
            assert not np.isnan(_value(r)).any(), "%s output %d: NaN left in the 256-CU result" % (what, i)
    for ncu, f in plans.items():   # (for the test report: the tile loop each share ran)
        print("%s ncu %d: tiles %d grid %d rounds %d cfg %d ksplit %d cgrp %d" % (what, ncu, f["tiles"], f["grid"], f["rounds"], f["cfg"], f["ksplit"], f["cgrp"]))
    return ref, plans


@pytest.fixture
def plan_debug(monkeypatch):
    monkeypatch.setenv("RSU_PLAN_DEBUG", "1")


# ------------------------------------------------------------------------------------------- conv forward
# starting shapes of the op tests, grown until the plan at 32 CUs (tiles of up to 640 pixels for Cout <= 64, up to 320 above) has three
# rounds and a short last one: N x Ho x Wo of about 3 x 32 x 640 pixels for one channel block, 3 x 16 x 320 for two
FWD_SHAPES = [
    # N, H, W, Cin, Cout, dil
    (2, 150, 140, 64, 64, 1),
    (1, 132, 130, 64, 192, 1),   # two channel blocks, the second half full
    (1, 146, 136, 96, 128, 2),
    (2, 164, 110, 16, 16, 1),    # channel counts that are no multiples of 32
]


@pytest.mark.parametrize("N,H,W,Cin,Cout,dil", FWD_SHAPES)
@pytest.mark.parametrize("relu", [1, 0])
def test_conv2d_fwd_every_share(N, H, W, Cin, Cout, dil, relu, capfd, plan_debug):
    rng = np.random.RandomState(Cin * 7 + Cout + H)
    x = hu.q(_rand(rng, N, H, W, Cin))
    w = _rand(rng, 3, 3, Cin, Cout, scale=1.0 / np.sqrt(9 * Cin))
    b = _rand(rng, Cout, scale=0.1)
    xd, wp, bd = hu.dev_bf16(x), hu.pack_conv_fwd(w), hu.dev_f32(b)
    Ho, Wo = H - 2 * dil, W - 2 * dil
    s = (RsuSrc * 1)(hu.src_of(xd, H, W))

    def launch(ncu):
        y = _nan(N, Ho, Wo, Cout)
        call("rsu_conv2d_fwd", s, 1, hu.ptr(wp), hu.ptr(bd), hu.ptr(y), N, H, W, Cout, dil, relu, ncu, hu.stream())
        return (y,)

    (y256,), plans = _across_shares(capfd, "conv2d_fwd", launch)
    hu.assert_bf16_close(_value(y256), U.conv2d_fwd(x, hu.q(w), b, dil=dil, relu=bool(relu)), "conv2d_fwd at 256 CUs")
    _assert_tile_loop_ran(plans[32], "conv2d_fwd")


@pytest.mark.parametrize("dil,h", [(1, 104), (2, 106)])
def test_conv2d_fwd_three_cropped_sources_every_share(dil, h, capfd, plan_debug):
    """the [48, 16, 64]-channel crop + concat of test_dilated_three_source_and_accumulate_every_shape, grown to three rounds at 32 CUs"""
    rng = np.random.RandomState(9 + dil)
    N, w, Cout = 2, 88, 128
    a = hu.q(_rand(rng, N, h + 12, w + 10, 48))
    bsrc = hu.q(_rand(rng, N, h + 6, w + 4, 16))
    c = hu.q(_rand(rng, N, h, w, 64))
    W = _rand(rng, 3, 3, 128, Cout, scale=0.05)
    bias = _rand(rng, Cout, scale=0.1)
    ad, bd_, cd, biasd = hu.dev_bf16(a), hu.dev_bf16(bsrc), hu.dev_bf16(c), hu.dev_f32(bias)
    wp = hu.pack_conv_fwd(W, [48, 16, 64])
    srcs = (RsuSrc * 3)(hu.src_of(ad, h, w), hu.src_of(bd_, h, w), hu.src_of(cd, h, w))

    def launch(ncu):
        y = _nan(N, h - 2 * dil, w - 2 * dil, Cout)
        call("rsu_conv2d_fwd", srcs, 3, hu.ptr(wp), hu.ptr(biasd), hu.ptr(y), N, h, w, Cout, dil, 1, ncu, hu.stream())
        return (y,)

    (y256,), plans = _across_shares(capfd, "3-source conv dil %d" % dil, launch)
    cat = np.concatenate([U.center_crop(a, h, w), U.center_crop(bsrc, h, w), c], axis=3)
    hu.assert_bf16_close(_value(y256), U.conv2d_fwd(cat, hu.q(W), bias, dil=dil), "3-source conv dil %d at 256 CUs" % dil)
    _assert_tile_loop_ran(plans[32], "3-source conv dil %d" % dil)


# ------------------------------------------------------------------------------------------- conv backward data
def test_conv2d_bwd_data_relu_mask_every_share(capfd, plan_debug):
    """ReluGrad of the producing layer in the epilogue; 72 gradient channels: a partial last 32-channel chunk of the reduction"""
    N, H, W, Cin, Cout = 3, 142, 96, 64, 72
    rng = np.random.RandomState(Cin + Cout * 3 + W)
    dz = hu.q(_rand(rng, N, H - 2, W - 2, Cout))
    w = _rand(rng, 3, 3, Cin, Cout, scale=1.0 / np.sqrt(9 * Cout))
    yprev = hu.q(np.maximum(_rand(rng, N, H, W, Cin), 0))
    wb, dzd, yd = hu.pack_conv_bwd(w), hu.dev_bf16(dz), hu.dev_bf16(yprev)

    def launch(ncu):
        dx = _nan(N, H, W, Cin)
        call("rsu_conv2d_bwd_data", hu.ptr(dzd), hu.ptr(wb), hu.ptr(dx), hu.ptr(yd), 0, N, H, W, Cin, 0, Cin, Cout, 1, ncu, hu.stream())
        return (dx,)

    (dx256,), plans = _across_shares(capfd, "bwd_data + relu mask", launch)
    hu.assert_bf16_close(_value(dx256), U.relu_bwd(yprev, U.conv2d_bwd_data(dz, hu.q(w), (H, W))), "bwd_data + relu mask at 256 CUs")
    _assert_tile_loop_ran(plans[32], "bwd_data + relu mask")


def test_conv2d_bwd_data_accumulate_dilated_every_share(capfd, plan_debug):
    """dx = base + Conv2DBackpropInput(dz) at dilation 2 (the dilated branch adding onto the main branch's input gradient)"""
    N, H, W, Cin, Cout = 2, 130, 88, 64, 128
    rng = np.random.RandomState(19)
    Wb = _rand(rng, 3, 3, Cin, Cout, scale=0.05)
    dz = hu.q(_rand(rng, N, H - 4, W - 4, Cout, scale=0.1))
    base = hu.q(_rand(rng, N, H, W, Cin, scale=0.1))
    dzd, wb, based = hu.dev_bf16(dz), hu.pack_conv_bwd(Wb, 0, Cin), hu.dev_bf16(base)

    def launch(ncu):
        dx = based.clone()
        call("rsu_conv2d_bwd_data", hu.ptr(dzd), hu.ptr(wb), hu.ptr(dx), None, 1, N, H, W, Cin, 0, Cin, Cout, 2, ncu, hu.stream())
        return (dx,)

    (dx256,), plans = _across_shares(capfd, "accumulating bwd_data dil 2", launch)
    hu.assert_bf16_close(_value(dx256), base + U.conv2d_bwd_data(dz, hu.q(Wb), (H, W), dil=2), "accumulating bwd_data dil 2 at 256 CUs")
    _assert_tile_loop_ran(plans[32], "accumulating bwd_data dil 2")


def test_conv2d_bwd_data_source_slice_every_share(capfd, plan_debug):
    """the gradient towards input channels [32, 96) of a conv with 128 inputs, from the pack of the whole kernel (tile_off in the kernels)"""
    N, H, W, Cin, Cout, off, cnt = 3, 102, 100, 128, 64, 32, 64
    rng = np.random.RandomState(29)
    dz = hu.q(_rand(rng, N, H - 2, W - 2, Cout))
    w = _rand(rng, 3, 3, Cin, Cout, scale=1.0 / np.sqrt(9 * Cout))
    wb, dzd = hu.pack_conv_bwd(w, 0, Cin), hu.dev_bf16(dz)

    def launch(ncu):
        dx = _nan(N, H, W, cnt)
        call("rsu_conv2d_bwd_data", hu.ptr(dzd), hu.ptr(wb), hu.ptr(dx), None, 0, N, H, W, Cin, off, cnt, Cout, 1, ncu, hu.stream())
        return (dx,)

    (dx256,), plans = _across_shares(capfd, "bwd_data slice", launch)
    hu.assert_bf16_close(_value(dx256), U.conv2d_bwd_data(dz, hu.q(w), (H, W))[..., off:off + cnt], "bwd_data slice at 256 CUs")
    _assert_tile_loop_ran(plans[32], "bwd_data slice")


# ------------------------------------------------------------------------------------------- conv + pool
@pytest.mark.parametrize("N,H,W,Cin,Cout,with_code", [(2, 146, 146, 64, 64, True), (1, 164, 130, 64, 128, True), (2, 163, 127, 32, 64, False)])
def test_conv2d_fwd_pool_every_share(N, H, W, Cin, Cout, with_code, capfd, plan_debug):
    """activation, pooled tensor and code bytes are the same at every share, whichever of the folded epilogue and the two launches a
    share's plan takes (the odd size: always the two launches, floor semantics, no code bytes)"""
    rng = np.random.RandomState(N * 7 + H + Cout)
    x = hu.q(_rand(rng, N, H, W, Cin))
    w = _rand(rng, 3, 3, Cin, Cout, scale=1.0 / np.sqrt(9 * Cin))
    b = _rand(rng, Cout, scale=0.1)
    xd, wp, bd = hu.dev_bf16(x), hu.pack_conv_fwd(w), hu.dev_f32(b)
    Ho, Wo = H - 2, W - 2
    Hp, Wp = Ho // 2, Wo // 2
    s = (RsuSrc * 1)(hu.src_of(xd, H, W))

    def launch(ncu):
        y, pooled = _nan(N, Ho, Wo, Cout), _nan(N, Hp, Wp, Cout)
        code = torch.full((N, Hp, Wp, Cout), 0xAA, dtype=torch.uint8, device=hu.DEV) if with_code else None
        call("rsu_conv2d_fwd_pool", s, 1, hu.ptr(wp), hu.ptr(bd), hu.ptr(y), hu.ptr(pooled), hu.ptr(code), N, H, W, Cout, 1.0, 0, ncu, hu.stream())
        return (y, pooled, code) if with_code else (y, pooled)

    outs, plans = _across_shares(capfd, "conv2d_fwd_pool", launch)
    y = _value(outs[0])
    hu.assert_bf16_close(y, U.conv2d_fwd(x, hu.q(w), b), "conv2d_fwd_pool activation at 256 CUs")
    np.testing.assert_array_equal(_value(outs[1]), U.maxpool_fwd(y), err_msg="pooled tensor is not the 2x2 max of the activation")
    if with_code:   # rsu.h: bits 0-3 = (window element 2*dy+dx > 0), bits 4-5 = the window's first maximum in row-major order
        win = y.reshape(N, Hp, 2, Wp, 2, Cout).transpose(0, 1, 3, 5, 2, 4).reshape(N, Hp, Wp, Cout, 4)
        ref_code = ((win > 0) * np.array([1, 2, 4, 8])).sum(-1) | (np.argmax(win, axis=-1) << 4)
        np.testing.assert_array_equal(outs[2], ref_code.astype(np.uint8), err_msg="code bytes")
    _assert_tile_loop_ran(plans[32], "conv2d_fwd_pool")


# ------------------------------------------------------------------------------------------- split-K
def test_conv2d_fwd_split_k_every_share(capfd, plan_debug):
    """a split launch has one tile slice per workgroup and its slice count is a function of the geometry alone: the same ksplit on the plan
    line and the same bits at every share"""
    N, H, W, segs, Cout = SPLITK_SHAPES[1]   # three concat sources, slices that start inside the 2nd / 3rd
    rng = np.random.RandomState(H * 7 + Cout + len(segs))
    Cin = sum(segs)
    xs = [hu.q(_rand(rng, N, H, W, c)) for c in segs]
    w = _rand(rng, 3, 3, Cin, Cout, scale=1.0 / np.sqrt(9 * Cin))
    b = _rand(rng, Cout, scale=0.1)
    xds = [hu.dev_bf16(x) for x in xs]
    wp, bd = hu.pack_conv_fwd(w, segs), hu.dev_f32(b)
    srcs = (RsuSrc * len(segs))(*[hu.src_of(xd, H, W) for xd in xds])
    nk = int(lib().rsu_conv_splitk_ws_floats())
    kws = _nan(nk, dtype=torch.float32)

    def launch(ncu):
        y = _nan(N, H - 2, W - 2, Cout)
        call("rsu_conv2d_fwd_k", srcs, len(segs), hu.ptr(wp), hu.ptr(bd), hu.ptr(y), N, H, W, Cout, 1, 1, ncu, hu.ptr(kws), nk, hu.stream())
        return (y,)

    (y256,), plans = _across_shares(capfd, "conv2d_fwd split-K", launch)
    assert plans[256]["ksplit"] > 1, plans[256]["line"]
    assert {p["ksplit"] for p in plans.values()} == {plans[256]["ksplit"]}, [p["line"] for p in plans.values()]
    hu.assert_bf16_close(_value(y256), U.conv2d_fwd(np.concatenate(xs, axis=3), hu.q(w), b), "conv2d_fwd split-K at 256 CUs")


def test_conv2d_bwd_data_split_k_every_share(capfd, plan_debug):
    N, H, W, segs, Cout = SPLITK_SHAPES[0]
    Cin = segs[0]
    rng = np.random.RandomState(Cin + Cout * 3 + W)
    dz = hu.q(_rand(rng, N, H - 2, W - 2, Cout))
    w = _rand(rng, 3, 3, Cin, Cout, scale=1.0 / np.sqrt(9 * Cout))
    yprev = hu.q(np.maximum(_rand(rng, N, H, W, Cin), 0))
    wb, dzd, yd = hu.pack_conv_bwd(w), hu.dev_bf16(dz), hu.dev_bf16(yprev)
    nk = int(lib().rsu_conv_splitk_ws_floats())
    kws = _nan(nk, dtype=torch.float32)

    def launch(ncu):
        dx = _nan(N, H, W, Cin)
        call("rsu_conv2d_bwd_data_k", hu.ptr(dzd), hu.ptr(wb), hu.ptr(dx), hu.ptr(yd), 0, N, H, W, Cin, 0, Cin, Cout, 1, ncu, hu.ptr(kws), nk, hu.stream())
        return (dx,)

    (dx256,), plans = _across_shares(capfd, "conv2d_bwd_data split-K", launch)
    assert plans[256]["ksplit"] > 1, plans[256]["line"]
    assert {p["ksplit"] for p in plans.values()} == {plans[256]["ksplit"]}, [p["line"] for p in plans.values()]
    hu.assert_bf16_close(_value(dx256), U.relu_bwd(yprev, U.conv2d_bwd_data(dz, hu.q(w), (H, W))), "conv2d_bwd_data split-K at 256 CUs")


# ------------------------------------------------------------------------------------------- transposed conv (igemm_ct)
# igemm_ct has no plan line. Its workgroups walk ceil(N H W / 256) pixel tiles in steps of ncu / ncob (ncob column blocks of 128:
# ceil(2 Cout / 128) x 2 phases forward, ceil(Cin / 128) backward). Tiles (T) against that step (S) at 32 CUs, forward | backward-data:
#   (2, 100, 100, 256, 128): T =  79, S =  8 | 16   -> 10 | 5 rounds
#   (4,  80,  81,  64,  32): T = 102, S = 16 | 32   ->  7 | 4 rounds
#   (3,  90,  95,  96, 160): T = 101, S =  5 | 32   -> 21 | 4 rounds
# every T exceeds 3 S and is no multiple of S (a short last round): asserted below. (3, 61, 67, 64, 32) and (1, 90, 94, 96, 160), the sizes
# of test_gpu_ops, are too small for that with one column block at 32 CUs: grown
@pytest.mark.parametrize("N,H,W,Cin,Cout", [(2, 100, 100, 256, 128), (4, 80, 81, 64, 32), (3, 90, 95, 96, 160)])
def test_convT_fwd_and_bwd_data_every_share(N, H, W, Cin, Cout, capfd):
    T = -(-N * H * W // 256)
    for S in (32 // (2 * -(-2 * Cout // 128)), 32 // -(-Cin // 128)):
        assert T > 3 * S and T % S, (T, S)
    rng = np.random.RandomState(Cin + H)
    x = hu.q(np.maximum(_rand(rng, N, H, W, Cin), 0))
    K = _rand(rng, 2, 2, Cout, Cin, scale=1.0 / np.sqrt(Cin))
    b = _rand(rng, Cout, scale=0.1)
    dy = hu.q(_rand(rng, N, 2 * H, 2 * W, Cout, scale=0.1))
    pf = torch.zeros(4 * lib().rsu_packed_bytes(1, Cout, (ctypes.c_int * 1)(Cin), 1) // 2, dtype=torch.bfloat16, device=hu.DEV)
    pb = torch.zeros(lib().rsu_packed_bytes(4, Cin, (ctypes.c_int * 1)(Cout), 1) // 2, dtype=torch.bfloat16, device=hu.DEV)
    Kd, xd, bd, dyd = hu.dev_f32(K), hu.dev_bf16(x), hu.dev_f32(b), hu.dev_bf16(dy)
    call("rsu_pack_convT_fwd", hu.ptr(Kd), hu.ptr(pf), Cin, Cout, hu.stream())
    call("rsu_pack_convT_bwd", hu.ptr(Kd), hu.ptr(pb), Cin, Cout, hu.stream())

    def launch(ncu):
        y, dx = _nan(N, 2 * H, 2 * W, Cout), _nan(N, H, W, Cin)
        call("rsu_convT2x2_fwd", hu.ptr(xd), hu.ptr(pf), hu.ptr(bd), hu.ptr(y), N, H, W, Cin, Cout, ncu, hu.stream())
        call("rsu_convT2x2_bwd_data", hu.ptr(dyd), hu.ptr(pb), hu.ptr(dx), hu.ptr(xd), 1.0, N, H, W, Cin, Cout, ncu, hu.stream())
        return (y, dx)

    (y256, dx256), _ = _across_shares(capfd, "convT", launch, plan=False)
    hu.assert_bf16_close(_value(y256), U.convT_fwd(x, hu.q(K), b), "convT fwd at 256 CUs")
    hu.assert_bf16_close(_value(dx256), U.relu_bwd(x, U.convT_bwd(x, hu.q(K), dy)[0]), "convT bwd_data at 256 CUs")


# ------------------------------------------------------------------------------------------- first layer
@pytest.mark.parametrize("N,H,W,Cout,dil", [(2, 200, 203, 64, 1), (1, 64, 64, 160, 2)])
def test_first_conv_every_share_and_both_entry_points(N, H, W, Cout, dil, capfd):
    """rsu_conv_first_fwd on the 16-channel tensor and rsu_color_conv_first_fwd on the f32 input: the same bits at every share"""
    rng = np.random.RandomState(5 + H)
    x = rng.rand(N, H, W, 3).astype(np.float32)
    w0, b0 = _rand(rng, 3, 3, scale=0.5), _rand(rng, 3, scale=0.1)
    w1, b1 = _rand(rng, 3, 3, 3, Cout, scale=0.3), _rand(rng, Cout, scale=0.1)
    xd_, w0d, b0d, w1d, b1d = hu.dev_f32(x), hu.dev_f32(w0), hu.dev_f32(b0), hu.dev_f32(w1), hu.dev_f32(b1)
    in16 = torch.zeros((N, H, W, 16), dtype=torch.bfloat16, device=hu.DEV)
    pk1 = torch.zeros(lib().rsu_packed_first_bytes(Cout) // 2, dtype=torch.bfloat16, device=hu.DEV)
    call("rsu_pack_conv_first", hu.ptr(w1d), hu.ptr(pk1), Cout, hu.stream())
    call("rsu_color_adjust_fwd", hu.ptr(xd_), hu.ptr(w0d), hu.ptr(b0d), hu.ptr(in16), N * H * W, 1.0, 0, hu.stream())
    Ho, Wo = H - 2 * dil, W - 2 * dil

    def launch(ncu):
        ya, yb = _nan(N, Ho, Wo, Cout), _nan(N, Ho, Wo, Cout)
        call("rsu_conv_first_fwd", hu.ptr(in16), hu.ptr(pk1), hu.ptr(b1d), hu.ptr(ya), N, H, W, Cout, dil, ncu, hu.stream())
        call("rsu_color_conv_first_fwd", hu.ptr(xd_), hu.ptr(w0d), hu.ptr(b0d), hu.ptr(pk1), hu.ptr(b1d), hu.ptr(yb), N, H, W, Cout, dil, ncu, hu.stream())
        return (ya, yb)

    (ya, yb), _ = _across_shares(capfd, "first conv", launch, plan=False)
    _assert_same_bits(ya, yb, "rsu_color_conv_first_fwd", 256, ref_name="rsu_conv_first_fwd")
    # (the oracle's conv on the device's own bf16 net0, as in test_color_adjust_and_first_conv: a 1-ulp flip of net0 is not this kernel's)
    hu.assert_bf16_close(_value(ya), U.conv2d_fwd(hu.host(in16)[..., 0:3], hu.q(w1), b1, dil=dil), "first conv at 256 CUs")


# ------------------------------------------------------------------------------------------- weight gradients
# ping-pong kernel (128 gradient channels and more), the 64-wide one, dilation 2
@pytest.mark.parametrize("N,H,W,Cin,Cout,dil", [(2, 30, 30, 64, 128, 1), (3, 21, 37, 72, 136, 1), (2, 37, 41, 64, 64, 1), (3, 21, 37, 72, 56, 1),
                                                (2, 60, 60, 128, 128, 2)])
def test_conv2d_bwd_weight_at_the_shares_of_the_schedules(N, H, W, Cin, Cout, dil):
    """ncu sets the number of partial sums per output tile (rsu.h): per share against the oracle, repeatable bit for bit, inside its workspace"""
    rng = np.random.RandomState(H + Cout + dil)
    Ho, Wo = H - 2 * dil, W - 2 * dil
    x = hu.q(_rand(rng, N, H, W, Cin))
    dz = hu.q(_rand(rng, N, Ho, Wo, Cout, scale=0.1))
    xd, dzd = hu.dev_bf16(x), hu.dev_bf16(dz)
    ref_dw, ref_db = U.conv2d_bwd_weight(x, dz, dil=dil)
    nws = lib().rsu_conv2d_bwd_weight_ws_floats(Cin, Cin, Cout)
    s = hu.src_of(xd, H, W)
    for ncu in WGRAD_SHARES:
        first = None
        for rep in range(2):
            ws = torch.zeros(nws + 1024, dtype=torch.float32, device=hu.DEV)
            ws[nws:] = 777.0
            dw = _nan(3, 3, Cin, Cout, dtype=torch.float32)
            db = _nan(Cout, dtype=torch.float32)
            call("rsu_conv2d_bwd_weight", ctypes.byref(s), hu.ptr(dzd), hu.ptr(dw), hu.ptr(db), hu.ptr(ws), N, Ho, Wo, Cin, 0, Cout, dil, ncu, hu.stream())
            got = (hu.host(dw), hu.host(db))
            assert bool((ws[nws:] == 777.0).all()), "workspace overrun at ncu = %d" % ncu
            if first is None:
                first = got
                hu.assert_f32_close(got[0], ref_dw, "bwd_weight at ncu = %d" % ncu)
                hu.assert_f32_close(got[1], ref_db, "bias grad at ncu = %d" % ncu)
            else:
                assert np.array_equal(first[0].view(np.uint32), got[0].view(np.uint32)), "bwd_weight does not repeat at ncu = %d" % ncu
                assert np.array_equal(first[1].view(np.uint32), got[1].view(np.uint32)), "bias grad does not repeat at ncu = %d" % ncu


# ------------------------------------------------------------------------------------------- forced unit grouping
def _admitted_groups(ncob, ksplit):
    """the values of RSU_COB_GROUP pick_cob_group itself considers: divisors of the unit count that divide ncob or are multiples of it"""
    nck = ncob * ksplit
    return [a for a in range(1, nck + 1) if nck % a == 0 and (ncob % a == 0 or a % ncob == 0)]


def _forced_grouping(capfd, monkeypatch, what, launch, shares):
    monkeypatch.delenv("RSU_COB_GROUP", raising=False)
    ref, seen = None, []
    for ncu in shares:
        capfd.readouterr()
        bits = _bits(launch(ncu))
        f = _plan_fields(capfd)
        if ref is None:
            ref = bits
            assert not np.isnan(_value(ref)).any()
        _assert_same_bits(ref, bits, what + ", planner's grouping", ncu)
        ncob = -(-f["Cout"] // f["TN"])
        for force in [0] + _admitted_groups(ncob, f["ksplit"]):
            monkeypatch.setenv("RSU_COB_GROUP", str(force))
            capfd.readouterr()
            bits = _bits(launch(ncu))
            g = _plan_fields(capfd)
            monkeypatch.delenv("RSU_COB_GROUP")
            assert (g["cfg"], g["grid"], g["ksplit"]) == (f["cfg"], f["grid"], f["ksplit"]), (f["line"], g["line"])
            assert g["cgrp"] == force, "RSU_COB_GROUP=%d did not take effect: %s" % (force, g["line"])
            _assert_same_bits(ref, bits, "%s, RSU_COB_GROUP=%d" % (what, force), ncu, ref_name="the planner's grouping at %d CUs" % shares[0])
            seen.append((ncu, force))
    print("%s: forced (ncu, group): %s" % (what, seen))
    return ref, seen


def test_forced_unit_grouping_two_channel_blocks(capfd, monkeypatch, plan_debug):
    """RSU_COB_GROUP remaps workgroup id -> (pixel tile, channel block): every admitted grouping must cover every unit exactly once,
    at one tile per workgroup (256 CUs) and in the tile loop (32 CUs)"""
    N, H, W, Cin, Cout = 1, 130, 130, 64, 256
    rng = np.random.RandomState(41)
    x = hu.q(_rand(rng, N, H, W, Cin))
    w = _rand(rng, 3, 3, Cin, Cout, scale=1.0 / np.sqrt(9 * Cin))
    b = _rand(rng, Cout, scale=0.1)
    xd, wp, bd = hu.dev_bf16(x), hu.pack_conv_fwd(w), hu.dev_f32(b)
    s = (RsuSrc * 1)(hu.src_of(xd, H, W))

    def launch(ncu):
        y = _nan(N, H - 2, W - 2, Cout)
        call("rsu_conv2d_fwd", s, 1, hu.ptr(wp), hu.ptr(bd), hu.ptr(y), N, H, W, Cout, 1, 1, ncu, hu.stream())
        return y

    ref, seen = _forced_grouping(capfd, monkeypatch, "conv2d_fwd", launch, (256, 32))
    assert {a for _, a in seen} >= {0, 1, 2}, seen   # two channel blocks: all of a tile together, one per run, both
    hu.assert_bf16_close(_value(ref), U.conv2d_fwd(x, hu.q(w), b), "conv2d_fwd, planner's grouping")


def test_forced_unit_grouping_split_k(capfd, monkeypatch, plan_debug):
    """... and workgroup id -> (pixel tile, channel block, reduction slice) of a split launch"""
    N, H, W, segs, Cout = SPLITK_SHAPES[0]
    Cin = segs[0]
    rng = np.random.RandomState(43)
    x = hu.q(_rand(rng, N, H, W, Cin))
    w = _rand(rng, 3, 3, Cin, Cout, scale=1.0 / np.sqrt(9 * Cin))
    b = _rand(rng, Cout, scale=0.1)
    xd, wp, bd = hu.dev_bf16(x), hu.pack_conv_fwd(w), hu.dev_f32(b)
    s = (RsuSrc * 1)(hu.src_of(xd, H, W))
    nk = int(lib().rsu_conv_splitk_ws_floats())
    kws = _nan(nk, dtype=torch.float32)

    def launch(ncu):
        y = _nan(N, H - 2, W - 2, Cout)
        call("rsu_conv2d_fwd_k", s, 1, hu.ptr(wp), hu.ptr(bd), hu.ptr(y), N, H, W, Cout, 1, 1, ncu, hu.ptr(kws), nk, hu.stream())
        return y

    ref, seen = _forced_grouping(capfd, monkeypatch, "conv2d_fwd split-K", launch, (256,))
    assert len(seen) >= 4, seen   # (the launch did split: more units per tile than channel blocks)
    hu.assert_bf16_close(_value(ref), U.conv2d_fwd(x, hu.q(w), b), "conv2d_fwd split-K, planner's grouping")
