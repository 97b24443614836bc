"""-m gpu: every launching entry point of include/rsu.h inside a fenced arena (tests/fence_util.py). The buffer descriptors of the MFMA
kernels carry num_records = 0x7fffffff: the hardware checks no bound, every tile edge is a hand-written predicate, and the exact-size
torch tensors of the op tests sit in 512-byte allocator blocks among finite data. Here ONE allocation per case holds every device buffer;
payloads end at their last byte; everything around them is the 16-bit word 0x7FA5 (NaN as bf16 and as float32); workspaces and packed
buffers have EXACTLY the advertised size. Arena.check() after the launches asserts that every band byte and every input byte is
unchanged (a stray write); the outputs go through the comparisons of the op test the launch is copied from, which treat NaN as out of
tolerance (a stray read that reaches a result, an element never written). Each family runs its smallest existing shape and an AWKWARD
one -- input channels a multiple of 8 but not of 32, output channels that fill no tile, a pixel count that fills no pixel tile, N >= 2,
byte sizes that are no multiples of 512 -- asserted on the host from the case's own shape tuple (_awkward).

FENCED / NOT_FENCED / SIZES are the registry tests/test_fence_host.py checks against include/rsu.h without a GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import tiler_oracle as T  # noqa: E402
from oracle import unet_oracle as U  # noqa: E402
from tests import fence_util as F  # noqa: E402
from tests import hiputil as hu  # noqa: E402
from road_segmentation_unet_amd._lib import RsuSrc, RsuWgradJob, call, lib  # noqa: E402

MiB = 1 << 20


def _rand(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def _host(t):
    torch.cuda.synchronize()
    return t.detach().to(torch.float32).cpu().numpy()


def _awkward(N, npix, Cin, Cout, *tensors):
    """the awkward-shape properties, from the case's own numbers: a later edit cannot quietly make the shape round. npix: the pixels
    of the GEMM's pixel axis (all images); the smallest pixel step of any kernel here is 32, the smallest channel tile 64."""
    assert N >= 2 and Cin % 8 == 0 and Cin % 32 != 0 and Cout % 8 == 0 and Cout % 64 != 0 and npix % 32 != 0, (N, npix, Cin, Cout)
    for t in tensors:
        assert (t.numel() * t.element_size()) % 512 != 0, tuple(t.shape)


def _packed(name, taps, rows, segs, mult=1):
    """a packed weight buffer of exactly rsu_packed_bytes (mult = 4: the four matrices of a transposed conv's forward pack)"""
    seg = (ctypes.c_int * len(segs))(*segs)
    return F.out(name, (mult * lib().rsu_packed_bytes(taps, rows, seg, len(segs)) // 2,))


def _plan_lines(capfd):
    return [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[plan fwd2]")]


FORCED = [(c, g) for c in range(8) for g in (2, 4) if not (g == 4 and c >= 6)]   # test_gpu_cfg_matrix.forced_cfg
forced = pytest.mark.parametrize("cfg,gen", FORCED, ids=["cfg%d-gen%d" % cg for cg in FORCED])


# =========================================================================================== 3x3 convolutions
# N, H, W, Cin, Cout, dil, awkward
CONV = [(2, 13, 19, 24, 40, 1, True), (1, 17, 15, 72, 136, 2, False), (2, 37, 41, 64, 64, 1, False)]
CONV_MULTI = (2, 37, 41, 72, 136, 1, True)    # the awkward shape with several tiles per workgroup: the forced tile shapes, ncu = 32


def _conv_fwd(shape, relu, ncu=0, y_rows_short=0, x_rows_short=0, compare=True, capfd=None, placement="aligned"):
    """test_gpu_ops.test_conv2d_fwd's launch, the weights packed by rsu_pack_conv_fwd into a buffer of exactly rsu_packed_bytes.
    y_rows_short / x_rows_short: the positive controls -- the output / the input carved that many image rows shorter than the call says"""
    N, H, W, Cin, Cout, dil, awkward = shape
    rng = np.random.RandomState(Cin * 7 + Cout + H)
    x = hu.q(_rand(rng, N, H, W, Cin))
    w = _rand(rng, 3, 3, Cin, Cout, scale=1.0 / np.sqrt(9 * Cin))
    b = _rand(rng, Cout, scale=0.1)
    Ho, Wo = H - 2 * dil, W - 2 * dil
    A = F.Arena(hu.DEV, [F.bf16("x", x.reshape(-1)[:(N * H - x_rows_short) * W * Cin]), F.f32("w", w), _packed("wp", 9, Cout, [Cin]), F.f32("b", b),
                         F.out("y", ((N * Ho - y_rows_short) * Wo * Cout,))], placement=placement)
    if awkward:
        _awkward(N, N * Ho * Wo, Cin, Cout, A["x"], A["y"], A["b"])
    seg = (ctypes.c_int * 1)(Cin)
    call("rsu_pack_conv_fwd", hu.ptr(A["w"]), hu.ptr(A["wp"]), 3, Cin, Cout, seg, 1, hu.stream())
    s = (RsuSrc * 1)(RsuSrc(A["x"].data_ptr(), H, W, Cin, 0, 0))
    if capfd is not None:
        capfd.readouterr()
    call("rsu_conv2d_fwd", s, 1, hu.ptr(A["wp"]), hu.ptr(A["b"]), hu.ptr(A["y"]), N, H, W, Cout, dil, relu, ncu, hu.stream())
    what = "conv2d_fwd %s relu %d ncu %d" % (shape[:6], relu, ncu)
    if capfd is not None:    # (RSU_PLAN_DEBUG=1: a failure names the tile shape, kernel generation and CU budget that ran)
        what += " [%s; RSU_FWD_GEN=%s cu budget %d]" % ("; ".join(_plan_lines(capfd)), os.environ.get("RSU_FWD_GEN", "default"), lib().rsu_get_cu_budget())
    A.check(what)
    if compare:
        hu.assert_bf16_close(_host(A["y"]).reshape(N, Ho, Wo, Cout), U.conv2d_fwd(x, hu.q(w), b, dil=dil, relu=bool(relu)), what)


@pytest.mark.parametrize("shape", CONV, ids=str)
@pytest.mark.parametrize("relu", [1, 0])
def test_conv2d_fwd(shape, relu, capfd, monkeypatch):
    monkeypatch.setenv("RSU_PLAN_DEBUG", "1")
    _conv_fwd(shape, relu, capfd=capfd)


# ReLU on AND off wherever a stray read is the point: the hardware's max(NaN, 0) is 0, so behind a ReLU (or a ReLU mask) a stray read
# shows only where the reference is positive; without it every touched element is NaN
@forced
@pytest.mark.parametrize("relu", [0, 1])
def test_conv2d_fwd_every_forced_shape(cfg, gen, relu, monkeypatch, capfd):
    monkeypatch.setenv("RSU_FWD2_CFG", str(cfg))
    monkeypatch.setenv("RSU_FWD_GEN", str(gen))
    monkeypatch.setenv("RSU_PLAN_DEBUG", "1")
    _conv_fwd(CONV_MULTI, relu, capfd=capfd)


@pytest.mark.parametrize("relu", [0, 1])
def test_conv2d_fwd_ncu32(relu, capfd, monkeypatch):
    """many tiles per workgroup: the last round of the persistent loop"""
    monkeypatch.setenv("RSU_PLAN_DEBUG", "1")
    _conv_fwd(CONV_MULTI, relu, ncu=32, capfd=capfd)


def _crop_case(sizes, chans, h, w, Cout, seed):
    """sources of `chans` channels, source i an (H, W) = sizes[i] tensor whose centred (h, w) window the conv reads; everything outside
    the window is arena pattern (the oracle sees only the crop)"""
    rng = np.random.RandomState(seed)
    N = 2
    srcs = [hu.q(_rand(rng, N, H, W, c)) for (H, W), c in zip(sizes, chans)]
    Cin = sum(chans)
    Wt = _rand(rng, 3, 3, Cin, Cout, scale=0.05)
    bias = _rand(rng, Cout, scale=0.1)
    cat = np.concatenate([U.center_crop(a, h, w) for a in srcs], axis=3)
    return N, srcs, Cin, Wt, bias, cat


@pytest.mark.parametrize("sizes,chans,h,w,Cout", [([(34, 38), (28, 30), (22, 26)], [32, 32, 32], 22, 26, 64), ([(25, 29), (19, 23)], [16, 16], 19, 23, 16),
                                                  ([(29, 33), (23, 27), (21, 23)], [24, 40, 8], 21, 23, 40)], ids=["32+32+32", "16+16", "24+40+8"])
@pytest.mark.parametrize("relu", [0, 1])
def test_conv2d_fwd_cropped_sources(sizes, chans, h, w, Cout, relu, placement="aligned"):
    """test_gpu_ops.test_conv2d_fwd_three_cropped_sources / _odd_channel_segments, the margins of every source poisoned; 24+40+8 -> 40 is
    the awkward one"""
    N, srcs, Cin, Wt, bias, cat = _crop_case(sizes, chans, h, w, Cout, 5)
    A = F.Arena(hu.DEV, [F.bf16("src%d" % i, a) for i, a in enumerate(srcs)] + [F.f32("w", Wt), _packed("wp", 9, Cout, chans), F.f32("b", bias),
                                                                                F.out("y", (N, h - 2, w - 2, Cout))], placement=placement)
    if chans[0] % 32:
        _awkward(N, N * (h - 2) * (w - 2), chans[0], Cout, A["y"], *[A["src%d" % i] for i in range(len(srcs))])
    for i, (H, W) in enumerate(sizes):
        A.poison_outside("src%d" % i, (H - h) // 2, (W - w) // 2, h, w)
    seg = (ctypes.c_int * len(chans))(*chans)
    call("rsu_pack_conv_fwd", hu.ptr(A["w"]), hu.ptr(A["wp"]), 3, Cin, Cout, seg, len(chans), hu.stream())
    s = (RsuSrc * len(srcs))(*[hu.src_of(A["src%d" % i], h, w) for i in range(len(srcs))])
    call("rsu_conv2d_fwd", s, len(srcs), hu.ptr(A["wp"]), hu.ptr(A["b"]), hu.ptr(A["y"]), N, h, w, Cout, 1, relu, 0, hu.stream())
    A.check("conv2d_fwd cropped sources")
    hu.assert_bf16_close(_host(A["y"]), U.conv2d_fwd(cat, hu.q(Wt), bias, relu=bool(relu)), "conv2d_fwd cropped sources %s relu %d" % (chans, relu))


@pytest.mark.parametrize("relu", [0, 1])
def test_conv2d_fwd_k_split(relu, capfd, monkeypatch, placement="aligned"):
    """test_gpu_ops.test_conv2d_fwd_split_k at (1, 20, 20, [200, 120] -> 128): the split asserted on the plan line, the workspace exactly
    rsu_conv_splitk_ws_floats"""
    monkeypatch.setenv("RSU_PLAN_DEBUG", "1")
    N, H, W, segs, Cout = 1, 20, 20, [200, 120], 128
    rng = np.random.RandomState(H * 7 + Cout + len(segs))
    Cin = sum(segs)
    xs = [hu.q(_rand(rng, N, H, W, c)) for c in segs]
    w = _rand(rng, 3, 3, Cin, Cout, scale=1.0 / np.sqrt(9 * Cin))
    b = _rand(rng, Cout, scale=0.1)
    nk = int(lib().rsu_conv_splitk_ws_floats())
    A = F.Arena(hu.DEV, [F.bf16("x0", xs[0]), F.bf16("x1", xs[1]), F.f32("w", w), _packed("wp", 9, Cout, segs), F.f32("b", b),
                         F.out("y", (N, H - 2, W - 2, Cout)), F.ws("kws", nk)], placement=placement)
    seg = (ctypes.c_int * 2)(*segs)
    call("rsu_pack_conv_fwd", hu.ptr(A["w"]), hu.ptr(A["wp"]), 3, Cin, Cout, seg, 2, hu.stream())
    s = (RsuSrc * 2)(hu.src_of(A["x0"], H, W), hu.src_of(A["x1"], H, W))
    capfd.readouterr()
    call("rsu_conv2d_fwd_k", s, 2, hu.ptr(A["wp"]), hu.ptr(A["b"]), hu.ptr(A["y"]), N, H, W, Cout, 1, relu, 0, hu.ptr(A["kws"]), nk, hu.stream())
    lines = _plan_lines(capfd)
    assert lines and " ksplit1 " not in lines[-1], lines
    A.check("conv2d_fwd_k split-K")
    hu.assert_bf16_close(_host(A["y"]), U.conv2d_fwd(np.concatenate(xs, axis=3), hu.q(w), b, relu=bool(relu)), "conv2d_fwd_k split-K relu %d" % relu)


def _bwd_data(shape, mode, ncu=0, k=False, capfd=None, placement="aligned"):
    """test_gpu_ops.test_conv2d_bwd_data's launches: mode "mask" (ReLU mask), "plain", "accumulate" (onto a stored bf16 tensor)"""
    N, H, W, Cin, Cout, dil, awkward = shape
    rng = np.random.RandomState(Cin + Cout * 3 + W)
    Ho, Wo = H - 2 * dil, W - 2 * dil
    dz = hu.q(_rand(rng, N, Ho, Wo, Cout))
    w = _rand(rng, 3, 3, Cin, Cout, scale=1.0 / np.sqrt(9 * Cout))
    yprev = hu.q(np.maximum(_rand(rng, N, H, W, Cin), 0))
    base = hu.q(_rand(rng, N, H, W, Cin))
    specs = [F.bf16("dz", dz), F.f32("w", w), _packed("wp", 9, Cin, [Cout]), F.bf16("yprev", yprev),
             F.state("dx", base, torch.bfloat16) if mode == "accumulate" else F.out("dx", (N, H, W, Cin))]
    nk = int(lib().rsu_conv_splitk_ws_floats())
    if k:
        specs.append(F.ws("kws", nk))
    A = F.Arena(hu.DEV, specs, placement=placement)
    if awkward:
        _awkward(N, N * H * W, Cout, Cin, A["dz"], A["dx"])     # (the GEMM's input channels are Cout, its output channels Cin)
    call("rsu_pack_conv_bwd", hu.ptr(A["w"]), hu.ptr(A["wp"]), 3, Cin, 0, Cin, Cout, hu.stream())
    mask = hu.ptr(A["yprev"]) if mode == "mask" else None
    if k:
        capfd.readouterr()
        call("rsu_conv2d_bwd_data_k", hu.ptr(A["dz"]), hu.ptr(A["wp"]), hu.ptr(A["dx"]), mask, int(mode == "accumulate"), N, H, W, Cin, 0, Cin, Cout, dil, ncu,
             hu.ptr(A["kws"]), nk, hu.stream())
        lines = _plan_lines(capfd)
        assert lines and " ksplit1 " not in lines[-1], lines
    else:
        call("rsu_conv2d_bwd_data", hu.ptr(A["dz"]), hu.ptr(A["wp"]), hu.ptr(A["dx"]), mask, int(mode == "accumulate"), N, H, W, Cin, 0, Cin, Cout, dil, ncu,
             hu.stream())
    what = "conv2d_bwd_data%s %s %s" % ("_k" if k else "", shape[:6], mode)
    A.check(what)
    g = U.conv2d_bwd_data(dz, hu.q(w), (H, W), dil=dil)
    if mode == "accumulate":
        # q(stored + fp32 sum): against stored + the oracle's sum, as the op test's "accumulate" (which grants the device's own first rounding)
        hu.assert_bf16_close(_host(A["dx"]), base.astype(np.float64) + g, what, ulps=2.0)
    else:
        hu.assert_bf16_close(_host(A["dx"]), U.relu_bwd(yprev, g) if mode == "mask" else g, what)


@pytest.mark.parametrize("shape", CONV, ids=str)
@pytest.mark.parametrize("mode", ["mask", "plain", "accumulate"])
def test_conv2d_bwd_data(shape, mode):
    _bwd_data(shape, mode)


@forced
@pytest.mark.parametrize("mode", ["plain", "mask"])
def test_conv2d_bwd_data_every_forced_shape(cfg, gen, mode, monkeypatch):
    monkeypatch.setenv("RSU_FWD2_CFG", str(cfg))
    monkeypatch.setenv("RSU_FWD_GEN", str(gen))
    _bwd_data(CONV_MULTI, mode)


@pytest.mark.parametrize("mode", ["plain", "mask"])
def test_conv2d_bwd_data_ncu32(mode):
    _bwd_data(CONV_MULTI, mode, ncu=32)


@pytest.mark.parametrize("mode", ["plain", "mask"])
def test_conv2d_bwd_data_k_split(mode, capfd, monkeypatch):
    """test_gpu_ops.test_conv2d_bwd_data_split_k at (1, 20, 20, 512, 512)"""
    monkeypatch.setenv("RSU_PLAN_DEBUG", "1")
    _bwd_data((1, 20, 20, 512, 512, 1, False), mode, k=True, capfd=capfd)


def test_conv2d_bwd_data_source_slice(placement="aligned"):
    """test_gpu_ops.test_conv2d_bwd_data_source_slice, N = 2, 24 -> 40 + 24 + 8 channels: one pack and one launch per concat source"""
    rng = np.random.RandomState(9)
    N, H, W, Cin, Cout = 2, 13, 19, 72, 24
    dz = hu.q(_rand(rng, N, H - 2, W - 2, Cout))
    w = _rand(rng, 3, 3, Cin, Cout, scale=0.1)
    full = U.conv2d_bwd_data(dz, hu.q(w), (H, W))
    slices = [(0, 40), (40, 24), (64, 8)]
    A = F.Arena(hu.DEV, [F.bf16("dz", dz), F.f32("w", w)] + [_packed("wp%d" % off, 9, cnt, [Cout]) for off, cnt in slices]
                + [F.out("dx%d" % off, (N, H, W, cnt)) for off, cnt in slices], placement=placement)
    _awkward(N, N * H * W, Cout, 40, A["dz"], A["dx0"])
    for off, cnt in slices:
        call("rsu_pack_conv_bwd", hu.ptr(A["w"]), hu.ptr(A["wp%d" % off]), 3, Cin, off, cnt, Cout, hu.stream())
        call("rsu_conv2d_bwd_data", hu.ptr(A["dz"]), hu.ptr(A["wp%d" % off]), hu.ptr(A["dx%d" % off]), None, 0, N, H, W, cnt, 0, cnt, Cout, 1, 0, hu.stream())
    A.check("conv2d_bwd_data source slices")
    for off, cnt in slices:
        hu.assert_bf16_close(_host(A["dx%d" % off]), np.ascontiguousarray(full[..., off:off + cnt]), "conv2d_bwd_data source slice %d..%d" % (off, off + cnt))


POOL = [(2, 12, 14, 24, 40, True), (2, 70, 70, 64, 64, False)]     # N, H, W, Cin, Cout, awkward (even conv outputs: code bytes need them)


@pytest.mark.parametrize("shape", POOL, ids=str)
@pytest.mark.parametrize("with_code", [1, 0])
@pytest.mark.parametrize("k", [0, 1], ids=["plain", "k"])
def test_conv2d_fwd_pool(shape, with_code, k, monkeypatch, capfd, placement="aligned"):
    """test_gpu_ops.test_conv2d_fwd_pool_equals_conv_then_pool's launch with RSU_POOL_FUSED=2 (fold wherever a tile shape can), with and
    without code bytes, through rsu_conv2d_fwd_pool and rsu_conv2d_fwd_pool_k (workspace exactly rsu_conv_splitk_ws_floats). At
    both shapes the folded kernel is asserted on the plan line (pool1, one conv launch: cfg3, strip width 16). Activation against the
    oracle; pooled tensor and code bytes exactly, from the device's own activation by the rule of rsu.h."""
    N, H, W, Cin, Cout, awkward = shape
    monkeypatch.setenv("RSU_POOL_FUSED", "2")
    monkeypatch.setenv("RSU_PLAN_DEBUG", "1")
    rng = np.random.RandomState(N * 7 + H + Cout)
    x = hu.q(_rand(rng, N, H, W, Cin))
    w = _rand(rng, 3, 3, Cin, Cout, scale=1.0 / np.sqrt(9 * Cin))
    b = _rand(rng, Cout, scale=0.1)
    Ho, Wo = H - 2, W - 2
    nk = int(lib().rsu_conv_splitk_ws_floats())
    specs = [F.bf16("x", x), F.f32("w", w), _packed("wp", 9, Cout, [Cin]), F.f32("b", b), F.out("y", (N, Ho, Wo, Cout)),
             F.out("pool", (N, Ho // 2, Wo // 2, Cout))]
    if with_code:
        specs.append(F.out("code", (N, Ho // 2, Wo // 2, Cout), torch.uint8))
    if k:
        specs.append(F.ws("kws", nk))
    A = F.Arena(hu.DEV, specs, placement=placement)
    if awkward:
        _awkward(N, N * Ho * Wo, Cin, Cout, A["x"], A["y"], A["pool"])
    seg = (ctypes.c_int * 1)(Cin)
    call("rsu_pack_conv_fwd", hu.ptr(A["w"]), hu.ptr(A["wp"]), 3, Cin, Cout, seg, 1, hu.stream())
    s = (RsuSrc * 1)(hu.src_of(A["x"], H, W))
    code = hu.ptr(A["code"]) if with_code else None
    capfd.readouterr()
    if k:
        call("rsu_conv2d_fwd_pool_k", s, 1, hu.ptr(A["wp"]), hu.ptr(A["b"]), hu.ptr(A["y"]), hu.ptr(A["pool"]), code, N, H, W, Cout, 1.0, 0, 0,
             hu.ptr(A["kws"]), nk, hu.stream())
    else:
        call("rsu_conv2d_fwd_pool", s, 1, hu.ptr(A["wp"]), hu.ptr(A["b"]), hu.ptr(A["y"]), hu.ptr(A["pool"]), code, N, H, W, Cout, 1.0, 0, 0, hu.stream())
    lines = _plan_lines(capfd)
    assert len(lines) == 1 and lines[-1].endswith(" pool1"), lines      # ONE conv launch, the pool folded into it, at both shapes
    what = "conv2d_fwd_pool%s %s code %d" % ("_k" if k else "", shape[:5], with_code)
    A.check(what)
    y = _host(A["y"])
    hu.assert_bf16_close(y, U.conv2d_fwd(x, hu.q(w), b, relu=True), what)
    np.testing.assert_array_equal(_host(A["pool"]), U.maxpool_fwd(y), err_msg=what + ": pooled")     # the pool of the device's own activation: exact
    if with_code:
        np.testing.assert_array_equal(A["code"].cpu().numpy(), _pool_code(y), err_msg=what + ": code bytes")


def _pool_code(x):
    """rsu.h, rsu_maxpool2x2_fwd_code: bits 0-3 = (window element 2*dy+dx > 0), bits 4-5 = the window's first maximum in row-major order"""
    N, H, W, C = x.shape
    win = np.stack([x[:, dy:H // 2 * 2:2, dx:W // 2 * 2:2, :] for dy in (0, 1) for dx in (0, 1)], axis=0)
    bits = sum(((win[i] > 0).astype(np.uint8) << i) for i in range(4))
    return (bits | (np.argmax(win, axis=0).astype(np.uint8) << 4)).astype(np.uint8)


# ------------------------------------------------------------------------------------------- 3x3 weight gradients, bias gradient
def _wgrad(shape, ncu=0, crop=None, placement="aligned"):
    """test_gpu_ops.test_conv2d_bwd_weight_and_bias's launches: the workspace exactly rsu_conv2d_bwd_weight_ws_floats; rsu_bias_grad
    with exactly rsu_bias_grad_ws_floats where it admits the channel count. crop = (H0, W0): the source is a larger tensor, its margins
    poisoned"""
    N, H, W, Cin, Cout, dil, awkward = shape
    rng = np.random.RandomState(Cin * 3 + Cout + H)
    Ho, Wo = H - 2 * dil, W - 2 * dil
    H0, W0 = crop or (H, W)
    xfull = hu.q(_rand(rng, N, H0, W0, Cin))
    x = U.center_crop(xfull, H, W)
    dz = hu.q(_rand(rng, N, Ho, Wo, Cout, scale=0.1))
    bias_ok = 256 % (Cout // 8) == 0
    specs = [F.bf16("x", xfull), F.bf16("dz", dz), F.out("dw", (3, 3, Cin, Cout), torch.float32), F.out("db", (Cout,), torch.float32),
             F.ws("ws", lib().rsu_conv2d_bwd_weight_ws_floats(Cin, Cin, Cout))]
    if bias_ok:
        specs += [F.out("db2", (Cout,), torch.float32), F.ws("bws", lib().rsu_bias_grad_ws_floats(N * Ho * Wo, Cout))]
    A = F.Arena(hu.DEV, specs, placement=placement)
    if awkward:
        _awkward(N, N * Ho * Wo, Cin, Cout, A["x"], A["dz"], A["db"])
    if crop:
        A.poison_outside("x", (H0 - H) // 2, (W0 - W) // 2, H, W)
    s = hu.src_of(A["x"], H, W)
    call("rsu_conv2d_bwd_weight", ctypes.byref(s), hu.ptr(A["dz"]), hu.ptr(A["dw"]), hu.ptr(A["db"]), hu.ptr(A["ws"]), N, Ho, Wo, Cin, 0, Cout, dil, ncu, hu.stream())
    if bias_ok:
        call("rsu_bias_grad", hu.ptr(A["dz"]), hu.ptr(A["db2"]), hu.ptr(A["bws"]), N * Ho * Wo, Cout, hu.stream())
    what = "conv2d_bwd_weight %s ncu %d" % (shape[:6], ncu)
    A.check(what)
    ref_dw, ref_db = U.conv2d_bwd_weight(x, dz, dil=dil)
    hu.assert_f32_close(_host(A["dw"]), ref_dw, what)
    hu.assert_f32_close(_host(A["db"]), ref_db, what + ": bias grad fused in wgrad")
    if bias_ok:
        hu.assert_f32_close(_host(A["db2"]), ref_db, what + ": bias_grad")


@pytest.mark.parametrize("shape", CONV, ids=str)
def test_conv2d_bwd_weight_and_bias_grad(shape):
    _wgrad(shape)


@pytest.mark.parametrize("npix,C", [(3 * 37 * 41, 8), (3 * 37 * 41, 16), (2 * 11 * 17, 64), (7, 8), (1003, 2048)])
def test_bias_grad(npix, C, placement="aligned"):
    """rsu_bias_grad admits C with 256 % (C / 8) == 0 only, which none of the awkward conv shapes has: here alone, at odd pixel counts
    (more than one block, and fewer pixels than a block has rows), the smallest and the largest admitted C, the workspace exactly
    rsu_bias_grad_ws_floats"""
    assert npix % 2 == 1 or npix == 2 * 11 * 17
    assert 256 % (C // 8) == 0 and (C == 2048 or (npix * C * 2) % 512 != 0)
    rng = np.random.RandomState(npix % 1000 + C)
    dz = hu.q(_rand(rng, npix, C, scale=0.1))
    A = F.Arena(hu.DEV, [F.bf16("dz", dz), F.out("db", (C,), torch.float32), F.ws("ws", lib().rsu_bias_grad_ws_floats(npix, C))], placement=placement)
    call("rsu_bias_grad", hu.ptr(A["dz"]), hu.ptr(A["db"]), hu.ptr(A["ws"]), npix, C, hu.stream())
    A.check("bias_grad npix %d C %d" % (npix, C))
    hu.assert_f32_close(_host(A["db"]), dz.astype(np.float64).sum(0), "bias_grad npix %d C %d" % (npix, C))


WG_MULTI = (3, 21, 37, 72, 136, 1, True)     # test_pingpong_wgrad_gives_the_bits_of_igemm_wgrad's awkward shape
WG_64 = (3, 21, 37, 72, 56, 1, True)         # test_pingpong_wgrad_64's


@pytest.mark.parametrize("env,shape", [({"RSU_WG_GEN": "1"}, WG_MULTI), ({"RSU_WG_GEN": "2"}, WG_MULTI), ({"RSU_WG64": "1"}, WG_64), ({"RSU_WG64": "0"}, WG_64),
                                       ({"RSU_WG_CFG": "0"}, WG_MULTI)], ids=["gen1", "pingpong", "wg64", "wg64-off", "cfg0"])
def test_conv2d_bwd_weight_every_kernel(env, shape, monkeypatch):
    """igemm_wgrad (RSU_WG_GEN=1), the ping-pong kernel (the default at 128 gradient channels), the 64-wide one (RSU_WG64, at 56
    gradient channels) and the 64x64 shape where 128x64 is the default (RSU_WG_CFG=0)"""
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    _wgrad(shape)


@pytest.mark.parametrize("shape", [WG_MULTI, WG_64], ids=str)
def test_conv2d_bwd_weight_ncu32(shape):
    _wgrad(shape, ncu=32)


def test_conv2d_bwd_weight_cropped_source():
    """test_gpu_ops.test_conv2d_bwd_weight_cropped_sources: a 24-channel source cropped out of a larger tensor, margins poisoned"""
    _wgrad((2, 13, 19, 24, 40, 1, True), crop=(25, 29))


def test_wgrad_group(monkeypatch, placement="aligned"):
    """test_gpu_ops.test_wgrad_group_equals_single_launches' job set (ncu = 64) with the workspace exactly rsu_wgrad_group_ws_floats (a 4 MiB
    band behind it: the planner checks its own need on the host) and the device table exactly rsu_wgrad_group_table_bytes"""
    ncu = 64
    rng = np.random.RandomState(77 + ncu)
    N = 2
    # (kind, H, W, Cin_total, ci_off, src C, Cout, dil)
    jobspecs = [(0, 38, 38, 128, 0, 128, 128, 1), (0, 70, 52, 64, 0, 64, 64, 1), (0, 20, 20, 256, 0, 256, 512, 1), (0, 44, 44, 64, 0, 64, 128, 2),
                (0, 30, 30, 96, 32, 64, 192, 1), (1, 11, 13, 128, 0, 128, 64, 1), (0, 150, 26, 128, 0, 128, 128, 1), (0, 33, 47, 64, 0, 64, 64, 2)]
    specs, refs = [], []
    for i, (kind, H, W, cin_t, off, csrc, cout, dil) in enumerate(jobspecs):
        if kind == 0:
            Ho, Wo = H - 2 * dil, W - 2 * dil
            x = hu.q(_rand(rng, N, H, W, csrc))
            dz = hu.q(_rand(rng, N, Ho, Wo, cout, scale=0.1))
            specs += [F.bf16("x%d" % i, x), F.bf16("dz%d" % i, dz), F.state("dw%d" % i, np.zeros((3, 3, cin_t, cout), np.float32)),
                      F.out("db%d" % i, (cout,), torch.float32)]
            refs.append(U.conv2d_bwd_weight(x, dz, dil=dil))
        else:
            x = hu.q(_rand(rng, N, H, W, cin_t))
            dy = hu.q(_rand(rng, N, 2 * H, 2 * W, cout, scale=0.1))
            specs += [F.bf16("x%d" % i, x), F.bf16("dz%d" % i, dy), F.out("dw%d" % i, (2, 2, cout, cin_t), torch.float32), F.out("db%d" % i, (cout,), torch.float32)]
            refs.append(U.convT_bwd(x, np.zeros((2, 2, cout, cin_t), np.float32), dy, need_dx=False)[1:])
    nb = lib().rsu_wgrad_group_table_bytes()
    specs += [F.ws("ws", lib().rsu_wgrad_group_ws_floats(), band=4 * MiB), F.out("table", (nb,), torch.uint8)]
    A = F.Arena(hu.DEV, specs, placement=placement)
    jobs = []
    for i, (kind, H, W, cin_t, off, csrc, cout, dil) in enumerate(jobspecs):
        if kind == 0:
            jobs.append(RsuWgradJob(0, hu.src_of(A["x%d" % i], H, W), A["dz%d" % i].data_ptr(), A["dw%d" % i].data_ptr(), A["db%d" % i].data_ptr(),
                                    H - 2 * dil, W - 2 * dil, cin_t, off, cout, dil))
        else:
            jobs.append(RsuWgradJob(1, RsuSrc(A["x%d" % i].data_ptr(), H, W, cin_t, 0, 0), A["dz%d" % i].data_ptr(), A["dw%d" % i].data_ptr(),
                                    A["db%d" % i].data_ptr(), 0, 0, 0, 0, cout, 1))
    host = ctypes.create_string_buffer(nb)
    arr = (RsuWgradJob * len(jobs))(*jobs)
    assert lib().rsu_wgrad_group_plan(arr, len(jobs), hu.ptr(A["ws"]), N, ncu, host) == 0
    A["table"].copy_(torch.frombuffer(bytearray(host.raw), dtype=torch.uint8))
    given = A["table"].clone()
    call("rsu_wgrad_group_run", host, hu.ptr(A["table"]), hu.stream())
    A.check("wgrad_group_run")
    assert torch.equal(A["table"], given), "the device table was written"
    for i, ((kind, H, W, cin_t, off, csrc, cout, dil), (rdw, rdb)) in enumerate(zip(jobspecs, refs)):
        gdw, gdb = _host(A["dw%d" % i]), _host(A["db%d" % i])
        if kind == 0:
            hu.assert_f32_close(gdw[:, :, off:off + csrc], rdw, "group conv wgrad %d" % i)
            assert not gdw[:, :, :off].any() and not gdw[:, :, off + csrc:].any(), "rows outside the source were written"
        else:
            hu.assert_f32_close(gdw, rdw, "group convT wgrad %d" % i)
        hu.assert_f32_close(gdb, rdb, "group bias grad %d" % i)


# =========================================================================================== transposed convolution
CONVT = [(2, 7, 9, 72, 40, True), (3, 33, 31, 72, 64, False), (2, 52, 50, 96, 96, False), (1, 9, 11, 24, 16, False)]   # N, H, W, Cin, Cout, awkward


def _convT(shape, ncu=0, ws_slabs_short=0, compare=True, placement="aligned"):
    """test_gpu_ops.test_convT's launches: forward, backward-data with the ReLU mask, rsu_dropout_fwd and the backward-data behind it
    (out_scale = 1 / keep), the weight gradient with a workspace of exactly rsu_convT2x2_bwd_weight_ws_floats; both packs into buffers of
    exactly rsu_packed_bytes"""
    N, H, W, Cin, Cout, awkward = shape
    rng = np.random.RandomState(Cin + H)
    x = hu.q(np.maximum(_rand(rng, N, H, W, Cin), 0))
    K = _rand(rng, 2, 2, Cout, Cin, scale=1.0 / np.sqrt(Cin))
    b = _rand(rng, Cout, scale=0.1)
    dy = hu.q(_rand(rng, N, 2 * H, 2 * W, Cout, scale=0.1))
    nws = lib().rsu_convT2x2_bwd_weight_ws_floats(Cin, Cout)
    if ws_slabs_short:
        nws -= ws_slabs_short * (4 * Cout * Cin + Cout)
    A = F.Arena(hu.DEV, [F.bf16("x", x), F.f32("K", K), _packed("pf", 1, Cout, [Cin], mult=4), _packed("pb", 4, Cin, [Cout]), F.f32("b", b), F.bf16("dy", dy),
                         F.out("y", (N, 2 * H, 2 * W, Cout)), F.out("dx", (N, H, W, Cin)), F.out("xdrop", (N, H, W, Cin)), F.out("dx2", (N, H, W, Cin)),
                         F.out("dK", (2, 2, Cout, Cin), torch.float32), F.out("db", (Cout,), torch.float32), F.ws("ws", nws)], placement=placement)
    if awkward:
        _awkward(N, N * H * W, Cin, Cout, A["x"], A["y"], A["dy"], A["db"])
    st = hu.stream()
    what = "convT %s ncu %d" % (shape[:5], ncu)
    if compare:
        call("rsu_pack_convT_fwd", hu.ptr(A["K"]), hu.ptr(A["pf"]), Cin, Cout, st)
        call("rsu_pack_convT_bwd", hu.ptr(A["K"]), hu.ptr(A["pb"]), Cin, Cout, st)
        call("rsu_convT2x2_fwd", hu.ptr(A["x"]), hu.ptr(A["pf"]), hu.ptr(A["b"]), hu.ptr(A["y"]), N, H, W, Cin, Cout, ncu, st)
        call("rsu_convT2x2_bwd_data", hu.ptr(A["dy"]), hu.ptr(A["pb"]), hu.ptr(A["dx"]), hu.ptr(A["x"]), 1.0, N, H, W, Cin, Cout, ncu, st)
        keep, key = 0.8, 0x5EED0001
        inv = np.float32(1) / np.float32(keep)
        call("rsu_dropout_fwd", hu.ptr(A["x"]), hu.ptr(A["xdrop"]), x.size, keep, key, st)
        call("rsu_convT2x2_bwd_data", hu.ptr(A["dy"]), hu.ptr(A["pb"]), hu.ptr(A["dx2"]), hu.ptr(A["xdrop"]), float(inv), N, H, W, Cin, Cout, ncu, st)
    call("rsu_convT2x2_bwd_weight", hu.ptr(A["x"]), hu.ptr(A["dy"]), hu.ptr(A["dK"]), hu.ptr(A["db"]), hu.ptr(A["ws"]), N, H, W, Cin, Cout, ncu, st)
    A.check(what)
    if not compare:
        return
    hu.assert_bf16_close(_host(A["y"]), U.convT_fwd(x, hu.q(K), b), what + " fwd")
    rdx, rdK, rdb = U.convT_bwd(x, hu.q(K), dy)
    hu.assert_bf16_close(_host(A["dx"]), U.relu_bwd(x, rdx), what + " bwd_data")
    m = U.dropout_mask(x.shape, keep, key)
    np.testing.assert_array_equal(_host(A["xdrop"]), hu.q(x * m * inv))
    hu.assert_bf16_close(_host(A["dx2"]), U.relu_bwd(x, rdx * m * inv), what + " bwd_data with dropout")
    hu.assert_f32_close(_host(A["dK"]), rdK, what + " bwd_weight")
    hu.assert_f32_close(_host(A["db"]), rdb, what + " bias grad")


@pytest.mark.parametrize("shape", CONVT, ids=str)
def test_convT(shape):
    _convT(shape)


@pytest.mark.parametrize("env", [{"RSU_CT_GEN": "1"}, {"RSU_CT_GEN": "2"}, {"RSU_WGT_GEN": "1"}, {"RSU_WGT_GEN": "3"}], ids=lambda e: "-".join("%s=%s" % kv for kv in e.items()))
@pytest.mark.parametrize("shape", [CONVT[0], CONVT[2]], ids=str)
def test_convT_every_kernel(env, shape, monkeypatch):
    """igemm_ct and igemm_fwd2's tap launches (RSU_CT_GEN), igemm_wgt and the generic weight-gradient launch (RSU_WGT_GEN), at the awkward
    shape and at (2, 52, 50, 96 -> 96): the shape whose weight gradient once wrote 82 slabs into room for 64"""
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    _convT(shape)


def test_convT_ncu32():
    _convT(CONVT[1], ncu=32)


# =========================================================================================== first layer
FIRST = [(1, 5, 19, 8, 1, False), (3, 21, 50, 72, 1, True), (1, 40, 37, 16, 2, False)]     # N, H, W, Cout, dil, awkward


def _first(shape, ncu=0, placement="aligned"):
    """test_gpu_ops.test_color_adjust_and_first_conv's launches (keep = 0.8 at dilation 1) plus rsu_color_conv_first_fwd and
    rsu_color_adjust_bwd: the packed buffer exactly rsu_packed_first_bytes, the workspace exactly rsu_conv_first_bwd_ws_floats. The
    first layer's input channels are 3 (16 stored): the awkward property "a multiple of 8 but not of 32" holds for the stored tensor."""
    N, H, W, Cout, dil, awkward = shape
    rng = np.random.RandomState(11 + dil + H)
    key, keep = 0xC0FFEE11, (0.8 if dil == 1 else 1.0)
    x = rng.rand(N, H, W, 3).astype(np.float32)
    w0, b0 = _rand(rng, 3, 3, scale=0.5), _rand(rng, 3, scale=0.1)
    w1, b1 = _rand(rng, 3, 3, 3, Cout, scale=0.3), _rand(rng, Cout, scale=0.1)
    Ho, Wo = H - 2 * dil, W - 2 * dil
    dz = hu.q(_rand(rng, N, Ho, Wo, Cout, scale=0.1))
    A = F.Arena(hu.DEV, [F.f32("x", x), F.f32("w0", w0), F.f32("b0", b0), F.f32("w1", w1), F.f32("b1", b1), F.bf16("dz", dz),
                         F.out("in16", (N, H, W, 16)), F.out("in16k", (N, H, W, 16)), F.out("pk1", (lib().rsu_packed_first_bytes(Cout) // 2,)),
                         F.out("y", (N, Ho, Wo, Cout)), F.out("yb", (N, Ho, Wo, Cout)),
                         F.out("dw1", (3, 3, 3, Cout), torch.float32), F.out("gx", (9, 12, Cout), torch.float32), F.out("db", (Cout,), torch.float32),
                         F.ws("ws", lib().rsu_conv_first_bwd_ws_floats(Cout)), F.out("dW0", (3, 3), torch.float32), F.out("db0", (3,), torch.float32)], placement=placement)
    if awkward:
        _awkward(N, N * Ho * Wo, 16, Cout, A["x"], A["y"], A["dz"], A["db"])
    st = hu.stream()
    npix = N * H * W
    call("rsu_color_adjust_fwd", hu.ptr(A["x"]), hu.ptr(A["w0"]), hu.ptr(A["b0"]), hu.ptr(A["in16"]), npix, 1.0, 0, st)
    call("rsu_color_adjust_fwd", hu.ptr(A["x"]), hu.ptr(A["w0"]), hu.ptr(A["b0"]), hu.ptr(A["in16k"]), npix, keep, key, st)
    call("rsu_pack_conv_first", hu.ptr(A["w1"]), hu.ptr(A["pk1"]), Cout, st)
    call("rsu_conv_first_fwd", hu.ptr(A["in16k"]), hu.ptr(A["pk1"]), hu.ptr(A["b1"]), hu.ptr(A["y"]), N, H, W, Cout, dil, ncu, st)
    call("rsu_color_conv_first_fwd", hu.ptr(A["x"]), hu.ptr(A["w0"]), hu.ptr(A["b0"]), hu.ptr(A["pk1"]), hu.ptr(A["b1"]), hu.ptr(A["yb"]), N, H, W, Cout, dil, ncu, st)
    call("rsu_conv_first_bwd_weight", hu.ptr(A["in16k"]), hu.ptr(A["dz"]), hu.ptr(A["dw1"]), hu.ptr(A["gx"]), hu.ptr(A["db"]), hu.ptr(A["ws"]), N, H, W, Cout, dil, ncu, st)
    call("rsu_color_adjust_bwd", hu.ptr(A["gx"]), hu.ptr(A["w1"]), hu.ptr(A["dW0"]), hu.ptr(A["db0"]), Cout, 1.25, 0, st)
    what = "first layer %s ncu %d" % (shape[:5], ncu)
    A.check(what)
    m = U.dropout_mask((N, H, W, 3), keep, key) if keep < 1.0 else np.ones((N, H, W, 3), np.float32)
    got16 = _host(A["in16k"])
    net0 = U.conv1x1_fwd(x, w0, b0, sub=0.5) * m * (np.float32(1) / np.float32(keep))
    hu.assert_bf16_close(got16[..., 0:3], net0, what + ": color_adjust net0")
    for ci in range(3):
        for cj in range(3):
            hu.assert_bf16_close(got16[..., 4 + 3 * ci + cj], (x[..., ci] - 0.5) * m[..., cj], what + ": color_adjust xc*m")
    np.testing.assert_array_equal(got16[..., 13:16], m)
    assert not got16[..., 3].any()
    hu.assert_bf16_close(_host(A["y"]), U.conv2d_fwd(got16[..., 0:3], hu.q(w1), b1, dil=dil), what + ": conv_first_fwd")
    hu.assert_bf16_close(_host(A["yb"]), U.conv2d_fwd(_host(A["in16"])[..., 0:3], hu.q(w1), b1, dil=dil), what + ": color_conv_first_fwd")
    hu.assert_f32_close(_host(A["db"]), dz.reshape(-1, Cout).astype(np.float64).sum(0), what + ": db")
    hu.assert_f32_close(_host(A["dw1"]), U.conv2d_bwd_weight(got16[..., 0:3], dz, dil=dil)[0], what + ": dW")
    gx = _host(A["gx"])
    hu.assert_f32_close(gx, U.conv2d_bwd_weight(got16[..., 4:16], dz, dil=dil)[0].reshape(9, 12, Cout), what + ": gx")
    w9 = w1.reshape(9, 3, Cout).astype(np.float64)
    np.testing.assert_allclose(_host(A["dW0"]), np.einsum("tjo,tijo->ij", w9, gx[:, :9].reshape(9, 3, 3, Cout).astype(np.float64)) * 1.25, rtol=2e-5, atol=2e-5)
    np.testing.assert_allclose(_host(A["db0"]), np.einsum("tjo,tjo->j", w9, gx[:, 9:].astype(np.float64)) * 1.25, rtol=2e-5, atol=2e-5)


@pytest.mark.parametrize("shape", FIRST, ids=str)
def test_first_layer(shape):
    _first(shape)


@pytest.mark.parametrize("env", [{"RSU_WG1_GEN": "1"}, {"RSU_WG1_GEN": "2"}, {"RSU_FIRST_GEN": "0"}], ids=lambda e: "-".join("%s=%s" % kv for kv in e.items()))
def test_first_layer_every_kernel(env, monkeypatch):
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    _first(FIRST[1])


def test_first_layer_ncu32():
    _first(FIRST[1], ncu=32)


# =========================================================================================== element-wise kernels
def _up2(a):
    return np.repeat(np.repeat(a, 2, axis=1), 2, axis=2)


def _pool_junction(shape, dskip_rows_short=0, placement="aligned"):
    """test_gpu_ops.test_maxpool_fwd_and_junction_bwd's launches: the pool with and without dropout, with code bytes where the size is
    even, the gradient junction from the activation and from the code bytes. (1, 9, 11, 8) pools an odd size with floor semantics."""
    N, H, W, C = shape
    rng = np.random.RandomState(H + C)
    x = hu.q(np.maximum(_rand(rng, N, H, W, C), 0))
    x[0, :4, :4, :] = x[0, 0, 0, :]
    keep, key = 0.8, 0x1234ABCD
    Hs, Ws = H - 4, W - 6
    Hp, Wp = H // 2, W // 2
    dpool = hu.q(_rand(rng, N, Hp, Wp, C))
    dskip = hu.q(_rand(rng, N, Hs, Ws, C))
    even = H % 2 == 0 and W % 2 == 0
    # (dskip_rows_short: the positive control -- the skip gradient carved that many image rows shorter than the call says)
    specs = [F.bf16("x", x), F.bf16("dpool", dpool), F.bf16("dskip", dskip.reshape(-1)[:(N * Hs - dskip_rows_short) * Ws * C]), F.out("y", (N, Hp, Wp, C)),
             F.out("yd", (N, Hp, Wp, C)), F.out("dz", (N, H, W, C)), F.out("dzd", (N, H, W, C))]
    if even:
        specs += [F.out("y2", (N, Hp, Wp, C)), F.out("code", (N, Hp, Wp, C), torch.uint8), F.out("dz2", (N, H, W, C))]
    A = F.Arena(hu.DEV, specs, placement=placement)
    st = hu.stream()
    call("rsu_maxpool2x2_fwd", hu.ptr(A["x"]), hu.ptr(A["y"]), N, H, W, C, 1.0, 0, st)
    call("rsu_maxpool2x2_fwd", hu.ptr(A["x"]), hu.ptr(A["yd"]), N, H, W, C, keep, key, st)
    call("rsu_pool_skip_relu_bwd", hu.ptr(A["x"]), hu.ptr(A["dpool"]), hu.ptr(A["dskip"]), hu.ptr(A["dz"]), N, H, W, C, Hs, Ws, 1.0, key, st)
    call("rsu_pool_skip_relu_bwd", hu.ptr(A["x"]), hu.ptr(A["dpool"]), hu.ptr(A["dskip"]), hu.ptr(A["dzd"]), N, H, W, C, Hs, Ws, keep, key, st)
    if even:
        call("rsu_maxpool2x2_fwd_code", hu.ptr(A["x"]), hu.ptr(A["y2"]), hu.ptr(A["code"]), N, H, W, C, 1.0, key, st)
        call("rsu_pool_skip_relu_bwd_code", None, hu.ptr(A["code"]), hu.ptr(A["dpool"]), hu.ptr(A["dskip"]), hu.ptr(A["dz2"]), N, H, W, C, Hs, Ws, 1.0, key, st)
    what = "pool and junction %s" % (shape,)
    A.check(what)
    mk = U.dropout_mask((N, Hp, Wp, C), keep, key) * (np.float32(1) / np.float32(keep))
    np.testing.assert_array_equal(_host(A["y"]), U.maxpool_fwd(x), err_msg=what)
    np.testing.assert_array_equal(_host(A["yd"]), hu.q(U.maxpool_fwd(x) * mk), err_msg=what + " dropout")
    for name, dp in (("dz", dpool), ("dzd", dpool * mk)):
        g = np.zeros_like(x)
        g[:, :Hp * 2, :Wp * 2] += U.maxpool_bwd(x[:, :Hp * 2, :Wp * 2], dp)
        g += U.center_pad_like(dskip, x.shape)
        hu.assert_bf16_close(_host(A[name]), U.relu_bwd(x, g), what + ": pool_skip_relu_bwd " + name)
    if even:
        np.testing.assert_array_equal(_host(A["y2"]), U.maxpool_fwd(x), err_msg=what + " code launch")
        np.testing.assert_array_equal(A["code"].cpu().numpy(), _pool_code(x), err_msg=what + ": code bytes")
        assert torch.equal(A["dz"].view(torch.int16), A["dz2"].view(torch.int16)), "code-byte junction differs"


@pytest.mark.parametrize("shape", [(1, 9, 11, 8), (2, 12, 16, 64), (2, 10, 14, 24)], ids=str)
def test_pool_and_junction(shape):
    """(2, 10, 14, 24): the awkward one (no channel tile here: 24 channels are three 16-byte pieces per pixel)"""
    if shape[3] == 24:
        N, H, W, C = shape
        assert N >= 2 and C % 8 == 0 and C % 32 != 0 and (N * H * W * C * 2) % 512 != 0 and (N * (H // 2) * (W // 2) * C) % 512 != 0
    _pool_junction(shape)


@pytest.mark.parametrize("n", [8, 2 * 7 * 9 * 72, 1003 * 8])
def test_dropout_fwd(n, placement="aligned"):
    """rsu_dropout_fwd takes n % 8 == 0 only (rsu.h): 8 (one vector), an awkward tensor's count, and 8024 = 8 * 1003 elements, whose byte
    size is no multiple of 512 and whose vector count is odd"""
    assert n % 8 == 0 and (n == 8 or (2 * n) % 512 != 0)
    rng = np.random.RandomState(n % 1000)
    x = hu.q(_rand(rng, n))
    keep, key = 0.8, 0x5EED0001
    A = F.Arena(hu.DEV, [F.bf16("x", x), F.out("y", (n,))], placement=placement)
    call("rsu_dropout_fwd", hu.ptr(A["x"]), hu.ptr(A["y"]), n, keep, key, hu.stream())
    A.check("dropout_fwd n %d" % n)
    m = U.dropout_mask((n,), keep, key)
    np.testing.assert_array_equal(_host(A["y"]), hu.q(x * m * (np.float32(1) / np.float32(keep))))


def test_dropout_fwd_refuses_a_count_that_is_no_multiple_of_8(placement="aligned"):
    """the precondition n % 8 == 0 of rsu.h is held, not assumed: RSU_EINVAL before anything is launched or written"""
    x = hu.q(_rand(np.random.RandomState(1), 1003))
    A = F.Arena(hu.DEV, [F.bf16("x", x), F.out("y", (1003,))], placement=placement)
    for n in (1003, 1001, 7):
        assert lib().rsu_dropout_fwd(hu.ptr(A["x"]), hu.ptr(A["y"]), n, 0.8, 1, hu.stream()) == -22, n
    A.check("refused dropout_fwd")
    assert bool(torch.isnan(A["y"]).all()), "a refused call wrote its output"


# =========================================================================================== the heads
from tests.head_util import LAM, NPIX, SMOOTH, Ref, _inputs, _weight_map, _with_ignored  # noqa: E402

HEAD_C = [8, 16, 32, 64, 128, 256, 512]      # every C the heads admit (rsu_api: 8 .. 512, C / 8 a power of two)


def _hist_from_prob(prob, labels):
    prob = np.asarray(prob, np.float32)
    bins = np.minimum(255, (prob * np.float32(256)).astype(np.int64))
    return np.stack([np.bincount(bins[labels == l], minlength=256) for l in (0, 1)]).astype(np.int64)


@pytest.mark.parametrize("C", HEAD_C)
def test_heads(C, placement="aligned"):
    """npix = 3 * 37 * 41 (odd: no multiple of any block) at every admitted C: rsu_head_fwd, _fwd_bwd, _fwd_bwd_w (class weights, a weight
    map, ignored labels), rsu_head_dice_sums + _fwd_bwd_dice, rsu_head_eval -- the launches of test_gpu_ops.test_head,
    test_gpu_weighted_loss, test_gpu_dice_loss and test_gpu_validation, each workspace exactly its own size function's"""
    assert NPIX == 3 * 37 * 41 and NPIX % 2 == 1
    rng, act, w, b, labels = _inputs(C)
    class_w, pixel_w = (0.6, 2.5), _weight_map(rng)
    lab_i, ign = _with_ignored(rng, labels)
    inv = 1.0 / (2 * NPIX)
    L = lib()
    z = lambda name, *s: F.state(name, np.zeros(s, np.float32))  # noqa: E731
    o32 = lambda name, *s: F.out(name, s, torch.float32)  # noqa: E731
    specs = [F.bf16("act", act), F.f32("w", w), F.f32("b", b), F.raw("labels", labels), F.raw("labels_i", lab_i), F.f32("cw", np.asarray(class_w, np.float32)),
             F.f32("pw", pixel_w), o32("prob0", NPIX), o32("logits", NPIX, 2)]
    for k in ("a", "w", "d", "e"):
        specs += [o32("prob_" + k, NPIX)]
    for k in ("a", "w", "d"):
        specs += [F.out("dact_" + k, (NPIX, C)), o32("dw_" + k, C, 2), o32("db_" + k, 2), z("loss_" + k, 1), z("wsum_" + k, 1)]
    specs += [o32("prob_s", NPIX), o32("dsums", 3), z("esums", 5), F.state("hist", np.zeros((2, 256), np.int64)),
              F.ws("ws_a", L.rsu_head_ws_floats(NPIX, C)), F.ws("ws_w", L.rsu_head_w_ws_floats(NPIX, C)), F.ws("ws_d", L.rsu_head_dice_ws_floats(NPIX, C)),
              F.ws("ws_e", L.rsu_head_eval_ws_floats(NPIX, C))]
    A = F.Arena(hu.DEV, specs, placement=placement)
    p = lambda n: hu.ptr(A[n])  # noqa: E731
    st = hu.stream()
    call("rsu_head_fwd", p("act"), p("w"), p("b"), p("prob0"), p("logits"), NPIX, C, st)
    call("rsu_head_fwd_bwd", p("act"), p("w"), p("b"), p("labels"), p("prob_a"), p("loss_a"), p("dact_a"), p("dw_a"), p("db_a"), p("ws_a"), NPIX, C, inv, st)
    call("rsu_head_fwd_bwd_w", p("act"), p("w"), p("b"), p("labels_i"), p("cw"), p("pw"), p("prob_w"), p("loss_w"), p("wsum_w"), p("dact_w"), p("dw_w"),
         p("db_w"), p("ws_w"), NPIX, C, inv, st)
    call("rsu_head_dice_sums", p("act"), p("w"), p("b"), p("labels"), None, p("prob_s"), p("dsums"), p("ws_d"), NPIX, C, st)
    call("rsu_head_fwd_bwd_dice", p("act"), p("w"), p("b"), p("labels"), p("cw"), None, p("dsums"), LAM, SMOOTH, p("prob_d"), p("loss_d"), p("wsum_d"),
         p("dact_d"), p("dw_d"), p("db_d"), p("ws_d"), NPIX, C, inv, st)
    call("rsu_head_eval", p("act"), p("w"), p("b"), p("labels_i"), p("cw"), p("pw"), p("prob_e"), p("esums"), p("hist"), p("ws_e"), NPIX, C, st)
    what = "heads C=%d" % C
    A.check(what)
    ref_logits = U.conv1x1_fwd(act, w, b)
    rp = U.softmax_ce(ref_logits, labels)[0]
    hu.assert_f32_close(_host(A["logits"]), ref_logits, what + " logits", rtol=1e-5)
    for k in ("prob0", "prob_a", "prob_w", "prob_d", "prob_s", "prob_e"):
        hu.assert_f32_close(_host(A[k]), rp, what + " " + k, rtol=1e-4, atol_scale=1e-6)
    safe_pw = np.where(~ign, pixel_w, 1.0)
    refs = {"a": Ref(act, w, b, labels, None, None, inv, lam=0.0), "w": Ref(act, w, b, lab_i, class_w, safe_pw, inv, lam=0.0),
            "d": Ref(act, w, b, labels, class_w, None, inv)}
    for k, r in refs.items():
        hu.assert_bf16_close(_host(A["dact_" + k]), r.dact, what + " dact_" + k)
        hu.assert_f32_close(_host(A["dw_" + k]), r.dw, what + " dw_" + k)
        hu.assert_f32_close(_host(A["db_" + k]), r.db, what + " db_" + k)
        assert abs(float(_host(A["loss_" + k])[0]) - r.ce_sum) <= 2e-5 * abs(r.ce_sum), (k, r.ce_sum)
    assert abs(float(_host(A["wsum_w"])[0]) - refs["w"].wsum) <= 2e-5 * refs["w"].wsum
    hu.assert_f32_close(_host(A["dsums"]), refs["d"].sums, what + " dice sums", rtol=2e-5)
    rw = refs["w"]
    hu.assert_f32_close(_host(A["esums"]), np.array([rw.ce_sum, rw.wsum, rw.sums[0], rw.sums[1], rw.sums[2]]), what + " eval sums", rtol=2e-5)
    np.testing.assert_array_equal(A["hist"].cpu().numpy(), _hist_from_prob(A["prob_e"].cpu().numpy(), lab_i))


def test_border_map(placement="aligned"):
    """test_gpu_border_map's launch at its smallest geometries as one batch of every case tile, with a caller map and d2; the workspace
    exactly rsu_border_map_ws_bytes"""
    from road_segmentation_unet_amd import hostio
    from tests import border_util as bu
    for H, W in ((20, 20), (37, 41)):
        tiles = bu.case_tiles(H, W)
        labels = np.stack([tiles[n] for n in sorted(tiles)])
        N = labels.shape[0]
        rng = np.random.RandomState(H * W)
        mul = bu.mul_map(rng, labels)
        nws = int(lib().rsu_border_map_ws_bytes(N, H, W))
        A = F.Arena(hu.DEV, [F.raw("labels", labels), F.f32("mul", mul), F.out("out", (N, H, W), torch.float32), F.out("d2", (N, H, W), torch.int32),
                             F.ws("ws", nws, torch.uint8)], placement=placement)
        call("rsu_border_map", hu.ptr(A["labels"]), hu.ptr(A["mul"]), hu.ptr(A["out"]), hu.ptr(A["d2"]), hu.ptr(A["ws"]), N, H, W, 10.0, 5.0, hu.stream())
        A.check("border_map %dx%dx%d" % (N, H, W))
        torch.cuda.synchronize()
        rd2 = np.stack([bu.brute_d2(t) for t in labels])
        np.testing.assert_array_equal(A["d2"].cpu().numpy(), rd2)
        hout, hd2 = hostio.border_weight_map(labels, 10.0, 5.0, mul=mul)
        np.testing.assert_array_equal(A["out"].cpu().numpy().view(np.int32), hout.view(np.int32))     # (the host mirror restates it bit for bit)
        ref, _ = bu.brute_map(labels, 10.0, 5.0, mul=mul)
        assert float(np.abs(A["out"].cpu().numpy().astype(np.float64) - ref).max()) <= bu.tolerance(10.0, mul)


# =========================================================================================== optimizer passes
def _np_adam(w, m, v, g, alpha, beta1, beta2, epsilon, gscale):
    """tests/test_gpu_adam.np_adam"""
    f32 = np.float32
    gs = f32(gscale) * g.astype(f32)
    m = m + (gs - m) * (f32(1) - f32(beta1))
    v = v + (gs * gs - v) * (f32(1) - f32(beta2))
    w = w - (m * f32(alpha)) / (np.sqrt(v) + f32(epsilon))
    return w, m, v


OPT_N = [1003, 3, 5]     # 1003: float4s and a tail of three; 3: below a vector width; 5: one vector and a tail


@pytest.mark.parametrize("n", OPT_N)
def test_momentum_adam_ema_accumulate_norm(n, placement="aligned"):
    """rsu_momentum_step, rsu_adam_step, rsu_grad_norm (workspace exactly rsu_grad_norm_ws_floats, the 32-byte record exactly
    rsu_clip_state_bytes), rsu_ema_step (with and without the record), rsu_grad_accumulate (assign and add) on vectors of n floats that end
    at their last byte: the launches of test_gpu_ops.test_momentum_step, test_gpu_adam.test_adam_step_op, test_gpu_clip, test_gpu_ema,
    test_gpu_accum"""
    f32 = np.float32
    rng = np.random.RandomState(31 + n)
    w, a, g = _rand(rng, n), _rand(rng, n), _rand(rng, n, scale=1e-2)
    m, v = _rand(rng, n, scale=1e-2), (rng.rand(n) * 1e-4).astype(f32)
    ema, dst = _rand(rng, n), _rand(rng, n)
    L = lib()
    assert L.rsu_clip_state_bytes() == 32
    A = F.Arena(hu.DEV, [F.f32("g", g), F.state("w", w), F.state("acc", a), F.state("w2", w), F.state("m", m), F.state("v", v), F.f32("wconst", w),
                         F.state("ema", ema), F.state("ema2", ema), F.state("dst", dst), F.out("dst2", (n,), torch.float32),
                         F.ws("nws", L.rsu_grad_norm_ws_floats(n)), F.state("state", np.zeros(L.rsu_clip_state_bytes() // 4, np.int32))], placement=placement)
    p = lambda k: hu.ptr(A[k])  # noqa: E731
    st = hu.stream()
    alpha, b1, b2, eps, omd = 1.234e-3, 0.9, 0.999, 1e-8, 0.25
    call("rsu_momentum_step", p("w"), p("acc"), p("g"), 0.01, 0.9, 0.5, n, st)
    call("rsu_adam_step", p("w2"), p("m"), p("v"), p("g"), alpha, b1, b2, eps, 0.5, n, st)
    call("rsu_grad_norm", p("g"), n, 1e-3, p("nws"), p("state"), st)
    call("rsu_ema_step", p("ema"), p("wconst"), n, omd, None, st)
    call("rsu_ema_step", p("ema2"), p("wconst"), n, omd, p("state"), st)
    call("rsu_grad_accumulate", p("dst"), p("g"), n, 0, st)
    call("rsu_grad_accumulate", p("dst2"), p("g"), n, 1, st)
    what = "optimizer passes n %d" % n
    A.check(what)
    ra = f32(0.9) * a + f32(0.5) * g
    np.testing.assert_allclose(_host(A["acc"]), ra, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(_host(A["w"]), w - f32(0.01) * ra, rtol=1e-6, atol=1e-7)
    rw, rm, rv = _np_adam(w, m, v, g, f32(alpha), b1, b2, eps, 0.5)
    for k, r in (("w2", rw), ("m", rm), ("v", rv)):
        np.testing.assert_allclose(_host(A[k]), r, rtol=1e-6, atol=0, err_msg=k)
    rec = A["state"].cpu().numpy()
    sumsq = float(np.sum(g.astype(np.float64) ** 2))
    assert abs(float(rec.view(f32)[0]) - sumsq) <= 4e-6 * sumsq and int(rec[3]) == 1 and int(rec[4]) == 1 and int(rec[7]) == 0, rec
    rema = ema - (ema - w) * f32(omd)
    np.testing.assert_array_equal(_host(A["ema"]), rema)       # (per element, float32, this order, no contraction: rsu.h)
    np.testing.assert_array_equal(_host(A["ema2"]), rema)      # (a record without RSU_CLIP_NONFINITE behaves as NULL)
    np.testing.assert_array_equal(_host(A["dst"]), dst + g)
    np.testing.assert_array_equal(_host(A["dst2"]), g)


@pytest.mark.parametrize("mode", ["momentum", "adam", "momentum_clip", "adam_clip"])
def test_update_and_pack_tables(mode, placement="aligned"):
    """rsu_update_table_run and its Adam and clip variants over a table with one entry of every kind -- a 3x3 conv kernel of two concat
    sources (24 + 16 -> 40), a transposed-conv kernel (72 -> 40), the first conv (3 -> 72) and a plain range of 1003 floats -- against the
    numpy restatement of the step; then rsu_pack_table_run and the per-tensor rsu_pack_* calls from the NEW weights into buffers of
    their own: the three sets of packed copies must agree bit for bit (every buffer exactly rsu_packed_bytes / rsu_packed_first_bytes),
    and one conv per kind reads the copies the update pass wrote (in test_conv2d_fwd, test_convT and test_first_layer the per-tensor
    packs feed the kernels). The clip variants read the record rsu_grad_norm left for the plain range's gradient."""
    f32 = np.float32
    adam, clip = mode.startswith("adam"), mode.endswith("clip")
    rng = np.random.RandomState(len(mode))
    L = lib()
    segs, Cc = [24, 16], 40
    var = {"conv": _rand(rng, 3, 3, 40, Cc, scale=0.1), "convT": _rand(rng, 2, 2, 40, 72, scale=0.1), "first": _rand(rng, 3, 3, 3, 72, scale=0.3),
           "plain": _rand(rng, 1003)}
    grads = {k: _rand(rng, *t.shape, scale=1e-2) for k, t in var.items()}
    accs = {k: _rand(rng, *t.shape, scale=1e-2) for k, t in var.items()}
    vs = {k: (rng.rand(*t.shape) * 1e-4).astype(f32) for k, t in var.items()}
    specs = []
    for k in var:
        specs += [F.state("w_" + k, var[k]), F.state("a_" + k, accs[k]), F.f32("g_" + k, grads[k])]
        if adam:
            specs.append(F.state("v_" + k, vs[k]))
    packs = {"conv_fwd": (9, Cc, segs, 1), "conv_bwd0": (9, 24, [Cc], 1), "conv_bwd1": (9, 16, [Cc], 1), "convT_fwd": (1, 40, [72], 4), "convT_bwd": (4, 72, [40], 1)}
    for tag in ("u", "t", "s"):     # written by the update pass, by the pack table, by the single pack calls
        specs += [_packed("%s_%s" % (tag, k), *a) for k, a in packs.items()]
        specs.append(F.out(tag + "_first", (L.rsu_packed_first_bytes(72) // 2,)))
    esz, psz = L.rsu_update_table_entry_bytes(), L.rsu_pack_table_entry_bytes()
    specs += [F.out("utable", (esz * 4,), torch.uint8), F.out("ptable", (psz * 9,), torch.uint8), F.ws("nws", L.rsu_grad_norm_ws_floats(1003)),
              F.state("state", np.zeros(8, np.int32))]
    x = hu.q(_rand(rng, 2, 9, 11, 40))
    A = F.Arena(hu.DEV, specs, placement=placement)
    p = lambda k: hu.ptr(A[k])  # noqa: E731
    st = hu.stream()
    # ---- the update table
    host = ctypes.create_string_buffer(esz * 4)
    seg = (ctypes.c_int * 2)(*segs)
    bw = (ctypes.c_void_p * 2)(A["u_conv_bwd0"].data_ptr(), A["u_conv_bwd1"].data_ptr())
    bwT = (ctypes.c_void_p * 1)(A["u_convT_bwd"].data_ptr())
    assert L.rsu_update_table_add(host, 0, 0, p("w_conv"), p("a_conv"), p("g_conv"), p("u_conv_fwd"), bw, 40, Cc, seg, 2) == 1
    assert L.rsu_update_table_add(host, 1, 2, p("w_convT"), p("a_convT"), p("g_convT"), p("u_convT_fwd"), bwT, 72, 40, None, 0) == 1
    assert L.rsu_update_table_add(host, 2, 4, p("w_first"), p("a_first"), p("g_first"), p("u_first"), None, 3, 72, None, 0) == 1
    assert L.rsu_update_table_add_plain(host, 3, p("w_plain"), p("a_plain"), p("g_plain"), 1003) == 1
    if adam:
        for i, k in enumerate(var):
            assert L.rsu_update_table_set_second_slot(host, i, p("v_" + k)) == 0
    nb = ctypes.c_int(0)
    assert L.rsu_update_table_finish(host, 4, ctypes.byref(nb)) == 0
    A["utable"].copy_(torch.frombuffer(bytearray(host.raw), dtype=torch.uint8))
    utable = A["utable"].clone()
    gscale, scale = 0.5, 1.0
    alpha, b1, b2, eps = 1.234e-3, 0.9, 0.999, 1e-8
    # the copies an update table points at were packed once from the initial weights (rsu.h: the pass rewrites the elements that hold
    # weights; the zero padding of the fragment order is the first pack's)
    call("rsu_pack_conv_fwd", p("w_conv"), p("u_conv_fwd"), 3, 40, Cc, seg, 2, st)
    call("rsu_pack_conv_bwd", p("w_conv"), p("u_conv_bwd0"), 3, 40, 0, 24, Cc, st)
    call("rsu_pack_conv_bwd", p("w_conv"), p("u_conv_bwd1"), 3, 40, 24, 16, Cc, st)
    call("rsu_pack_convT_fwd", p("w_convT"), p("u_convT_fwd"), 72, 40, st)
    call("rsu_pack_convT_bwd", p("w_convT"), p("u_convT_bwd"), 72, 40, st)
    call("rsu_pack_conv_first", p("w_first"), p("u_first"), 72, st)
    torch.cuda.synchronize()
    old = {k: A["u_" + k].clone() for k in list(packs) + ["first"]}
    if clip:
        call("rsu_grad_norm", p("g_plain"), 1003, 0.05, p("nws"), p("state"), st)
        torch.cuda.synchronize()
        scale = float(A["state"].cpu().numpy().view(f32)[2])
        assert 0 < scale < 1
    if mode == "momentum":
        call("rsu_update_table_run", p("utable"), 4, nb.value, 0.01, 0.9, gscale, st)
    elif mode == "adam":
        call("rsu_update_table_run_adam", p("utable"), 4, nb.value, alpha, b1, b2, eps, gscale, st)
    elif mode == "momentum_clip":
        call("rsu_update_table_run_clip", p("utable"), 4, nb.value, 0.01, 0.9, gscale, p("state"), st)
    else:
        call("rsu_update_table_run_adam_clip", p("utable"), 4, nb.value, alpha, b1, b2, eps, gscale, p("state"), st)
    # ---- the same packs from the new weights: the pack table, the single calls
    ph = ctypes.create_string_buffer(psz * 9)
    idx = 0
    for kind, wk, pk, k_, cin, off, cnt, cout, sg in ((0, "w_conv", "t_conv_fwd", 3, 40, 0, 40, Cc, seg), (1, "w_conv", "t_conv_bwd0", 3, 40, 0, 24, Cc, None),
                                                      (1, "w_conv", "t_conv_bwd1", 3, 40, 24, 16, Cc, None), (2, "w_convT", "t_convT_fwd", 1, 72, 0, 72, 40, None),
                                                      (3, "w_convT", "t_convT_bwd", 1, 72, 0, 72, 40, None), (4, "w_first", "t_first", 3, 3, 0, 3, 72, None)):
        used = L.rsu_pack_table_add(ph, idx, kind, p(wk), p(pk), k_, cin, off, cnt, cout, sg, 2 if sg else 0)
        assert used >= 1, (pk, used)
        idx += used
    assert idx == 9
    pnb = ctypes.c_int(0)
    assert L.rsu_pack_table_finish(ph, idx, ctypes.byref(pnb)) == 0
    A["ptable"].copy_(torch.frombuffer(bytearray(ph.raw), dtype=torch.uint8))
    ptable = A["ptable"].clone()
    call("rsu_pack_table_run", p("ptable"), idx, pnb.value, st)
    call("rsu_pack_conv_fwd", p("w_conv"), p("s_conv_fwd"), 3, 40, Cc, seg, 2, st)
    call("rsu_pack_conv_bwd", p("w_conv"), p("s_conv_bwd0"), 3, 40, 0, 24, Cc, st)
    call("rsu_pack_conv_bwd", p("w_conv"), p("s_conv_bwd1"), 3, 40, 24, 16, Cc, st)
    call("rsu_pack_convT_fwd", p("w_convT"), p("s_convT_fwd"), 72, 40, st)
    call("rsu_pack_convT_bwd", p("w_convT"), p("s_convT_bwd"), 72, 40, st)
    call("rsu_pack_conv_first", p("w_first"), p("s_first"), 72, st)
    what = "update / pack tables, " + mode
    A.check(what)
    assert torch.equal(A["utable"], utable) and torch.equal(A["ptable"], ptable), "a device table was written"
    gs = f32(gscale) * f32(scale)
    for k in var:
        if adam:
            rw, rm, rv = _np_adam(var[k], accs[k], vs[k], grads[k], f32(alpha), b1, b2, eps, gs)
            for name, r in (("w_", rw), ("a_", rm), ("v_", rv)):
                np.testing.assert_allclose(_host(A[name + k]), r, rtol=1e-6, atol=0, err_msg=name + k)
        else:
            ra = f32(0.9) * accs[k] + gs * grads[k]
            np.testing.assert_allclose(_host(A["a_" + k]), ra, rtol=1e-6, atol=1e-7, err_msg=k)
            np.testing.assert_allclose(_host(A["w_" + k]), var[k] - f32(0.01) * ra, rtol=1e-6, atol=1e-7, err_msg=k)
    for k in list(packs) + ["first"]:
        u, t, s = (A["%s_%s" % (tag, k)].view(torch.int16) for tag in ("u", "t", "s"))
        assert not bool(torch.isnan(A["u_" + k].float()).any()), k
        assert torch.equal(u, s), "update pass against rsu_pack_*: " + k
        assert not torch.equal(u, old[k].view(torch.int16)), "the update pass left the old copy: " + k
        assert torch.equal(t, s), "rsu_pack_table_run against rsu_pack_*: " + k
    # ---- one conv on the copy the update pass wrote (its two sources and its output in an arena of their own)
    xa, xb = np.ascontiguousarray(x[..., :24]), np.ascontiguousarray(x[..., 24:])
    B = F.Arena(hu.DEV, [F.bf16("xa", xa), F.bf16("xb", xb), F.out("y", (2, 7, 9, Cc))], placement=placement)
    s2 = (RsuSrc * 2)(hu.src_of(B["xa"], 9, 11), hu.src_of(B["xb"], 9, 11))
    call("rsu_conv2d_fwd", s2, 2, p("u_conv_fwd"), None, hu.ptr(B["y"]), 2, 9, 11, Cc, 1, 1, 0, st)
    B.check(what + ": conv on the re-packed copy")
    A.check(what + ": conv on the re-packed copy")
    hu.assert_bf16_close(_host(B["y"]), U.conv2d_fwd(x, hu.q(_host(A["w_conv"])), None, relu=True), what + ": conv on the re-packed copy")


# =========================================================================================== host-path kernels
def test_tilers_square_and_rect(placement="aligned"):
    """test_gpu_ops.test_tiler_extract_and_overlap at (20, 8, 12, 4, 2) and test_gpu_tiler_rect.test_rect_tiler_against_the_rule at
    (2, 23, 31, 8, 12, 5), its smallest geometry with a clamped last tile; both in two calls split at nt // 2, then rsu_overlap_finish"""
    from tests import rect_util as R
    rng = np.random.RandomState(20)
    # square
    H, P, S, stride, nimg = 20, 8, 12, 4, 2
    imgs = rng.rand(nimg, H, H, 3).astype(np.float32)
    pps = (H - P) // stride + 1
    nt = nimg * pps * pps
    prob = rng.rand(nt, P, P).astype(np.float32)
    # rectangular
    nimg2, H2, W2, P2, S2, stride2 = 2, 23, 31, 8, 12, 5
    imgs2 = rng.rand(nimg2, H2, W2, 3).astype(np.float32)
    nt2 = len(R.tile_list(nimg2, H2, W2, P2, stride2))
    prob2 = rng.rand(nt2, P2, P2).astype(np.float32)
    zeros = lambda name, *s: F.state(name, np.zeros(s, np.float32))  # noqa: E731
    A = F.Arena(hu.DEV, [F.f32("imgs", imgs), F.f32("prob", prob), F.out("tiles", (nt, S, S, 3), torch.float32), zeros("acc", nimg, H, H), zeros("hits", nimg, H, H),
                         F.out("mean", (nimg, H, H), torch.float32),
                         F.f32("imgs2", imgs2), F.f32("prob2", prob2), F.out("tiles2", (nt2, S2, S2, 3), torch.float32), zeros("acc2", nimg2, H2, W2),
                         zeros("hits2", nimg2, H2, W2), F.out("mean2", (nimg2, H2, W2), torch.float32)], placement=placement)
    p = lambda k: hu.ptr(A[k])  # noqa: E731
    st = hu.stream()
    half = nt // 2
    call("rsu_extract_tiles", p("imgs"), p("tiles"), nimg, H, S, P, stride, 0, half, st)
    call("rsu_extract_tiles", p("imgs"), hu.ptr(A["tiles"][half:]), nimg, H, S, P, stride, half, nt - half, st)
    call("rsu_overlap_add", p("prob"), p("acc"), p("hits"), nimg, H, P, stride, 0, half, st)
    call("rsu_overlap_add", hu.ptr(A["prob"][half:]), p("acc"), p("hits"), nimg, H, P, stride, half, nt - half, st)
    call("rsu_overlap_finish", p("acc"), p("hits"), p("mean"), nimg * H * H, st)
    half2 = nt2 // 2
    call("rsu_extract_tiles_rect", p("imgs2"), p("tiles2"), nimg2, H2, W2, S2, P2, stride2, 0, half2, st)
    call("rsu_extract_tiles_rect", p("imgs2"), hu.ptr(A["tiles2"][half2:]), nimg2, H2, W2, S2, P2, stride2, half2, nt2 - half2, st)
    call("rsu_overlap_add_rect", p("prob2"), p("acc2"), p("hits2"), nimg2, H2, W2, P2, stride2, 0, half2, st)
    call("rsu_overlap_add_rect", hu.ptr(A["prob2"][half2:]), p("acc2"), p("hits2"), nimg2, H2, W2, P2, stride2, half2, nt2 - half2, st)
    call("rsu_overlap_finish", p("acc2"), p("hits2"), p("mean2"), nimg2 * H2 * W2, st)
    A.check("tilers")
    ref = T.extract_patches(T.mirror_border(imgs, (S - P) // 2), S, stride=stride, predict_patch_size=P)
    np.testing.assert_array_equal(_host(A["tiles"]), ref.astype(np.float32))
    refm = T.images_from_patches(prob.astype(np.float64).reshape(nimg, pps * pps, P, P, 1), stride=stride)[..., 0]
    np.testing.assert_allclose(_host(A["mean"]), refm, rtol=2e-6, atol=1e-7)
    np.testing.assert_array_equal(_host(A["tiles2"]), R.extract(imgs2, S2, P2, stride2))
    refm2, refh2 = R.overlap(prob2, nimg2, H2, W2, stride2)
    np.testing.assert_array_equal(_host(A["hits2"]), refh2.astype(np.float32))
    np.testing.assert_allclose(_host(A["mean2"]), refm2, rtol=2e-6, atol=1e-7)


def test_quantize_labels_confusion(placement="aligned"):
    """rsu_quantize_mask (40 px masks, 16 px blocks: edge blocks hold 8 of 16 pixels; out of place and in place), rsu_quantize_mask_rect
    (2, 40, 56), rsu_labels_for_patches (48 px, 16 px patches) and rsu_confusion_counts (n = 5003) against hostio's numpy statements"""
    from road_segmentation_unet_amd import hostio
    rng = np.random.RandomState(9)
    m = rng.rand(2, 40, 40, 1).astype(np.float32)
    m2 = rng.rand(2, 40, 56, 1).astype(np.float32)
    m3 = rng.rand(2, 48, 48).astype(np.float32)
    n = 5003
    pred, truth = (rng.rand(n) > 0.6).astype(np.int64), (rng.rand(n) > 0.5).astype(np.int64)
    A = F.Arena(hu.DEV, [F.f32("m", m[..., 0]), F.out("q", (2, 40, 40), torch.float32), F.state("m_inplace", m[..., 0]),
                         F.f32("m2", m2[..., 0]), F.out("q2", (2, 40, 56), torch.float32), F.state("m2_inplace", m2[..., 0]),
                         F.f32("m3", m3), F.out("lab", (2, 3, 3), torch.int64), F.raw("pred", pred), F.raw("truth", truth),
                         F.state("counts", np.zeros(4, np.int64))], placement=placement)
    p = lambda k: hu.ptr(A[k])  # noqa: E731
    st = hu.stream()
    call("rsu_quantize_mask", p("m"), p("q"), 2, 40, 16, 0.25, st)
    call("rsu_quantize_mask", p("m_inplace"), p("m_inplace"), 2, 40, 16, 0.25, st)
    call("rsu_quantize_mask_rect", p("m2"), p("q2"), 2, 40, 56, 16, 0.25, st)
    call("rsu_quantize_mask_rect", p("m2_inplace"), p("m2_inplace"), 2, 40, 56, 16, 0.25, st)
    call("rsu_labels_for_patches", p("m3"), p("lab"), 2, 48, 16, 0.25, st)
    call("rsu_confusion_counts", p("pred"), p("truth"), n, p("counts"), st)
    A.check("quantize / labels / confusion")
    want = hostio.quantize_mask(m, 0.25, 16)[..., 0].astype(np.float32)
    np.testing.assert_array_equal(_host(A["q"]), want)
    np.testing.assert_array_equal(_host(A["m_inplace"]), want)
    want2 = hostio.quantize_mask(m2, 0.25, 16)[..., 0].astype(np.float32)
    np.testing.assert_array_equal(_host(A["q2"]), want2)
    np.testing.assert_array_equal(_host(A["m2_inplace"]), want2)
    # labels_for_patches over extract_patches(mask, 16): x outer, y inner; label = mean(patch) > threshold
    blocks = m3.astype(np.float64).reshape(2, 3, 16, 3, 16).mean(axis=(2, 4))          # [n][by][bx]
    np.testing.assert_array_equal(A["lab"].cpu().numpy(), (blocks.transpose(0, 2, 1) > 0.25).astype(np.int64))
    tp, fp = int(((pred == 1) & (truth == 1)).sum()), int(((pred == 1) & (truth == 0)).sum())
    fn, tn = int(((pred == 0) & (truth == 1)).sum()), int(((pred == 0) & (truth == 0)).sum())
    np.testing.assert_array_equal(A["counts"].cpu().numpy(), [tp, fp, fn, tn])


def test_affine_and_elastic_patches(placement="aligned"):
    """rsu_affine_patches and rsu_elastic_patches at their own tests' smallest geometries, the bank's first 38 records (crosses the
    32-record cut): bit for bit against the host mirrors (tests/affine_util.py, tests/elastic_util.py)"""
    from road_segmentation_unet_amd import _lib, hostio
    from tests import affine_util as au
    from tests import elastic_util as eu
    Hl, offset, S, P = au.GEOMS[1]           # (20, 3, 11, 5): odd sizes
    ext, lab, recs, hx, hy = eu.affine_case(Hl, offset, S, P)
    n = 38
    recs = np.ascontiguousarray(recs[:n])
    _, _, erecs, ehx, ehy = eu.case(Hl, offset, S, P)
    erecs = np.ascontiguousarray(erecs[200:200 + n])
    A = F.Arena(hu.DEV, [F.f32("img", ext), F.raw("lab", np.ascontiguousarray(lab, dtype=np.uint8)), F.out("x", (n, S, S, 3), torch.float32),
                         F.out("y", (n, P, P), torch.int64), F.out("ex", (n, S, S, 3), torch.float32), F.out("ey", (n, P, P), torch.int64)], placement=placement)
    p = lambda k: hu.ptr(A[k])  # noqa: E731
    call("rsu_affine_patches", p("img"), p("lab"), recs.ctypes.data_as(ctypes.POINTER(_lib.RsuAffine)), n, ext.shape[0], ext.shape[1], lab.shape[1], S, P,
         p("x"), p("y"), hu.stream())
    call("rsu_elastic_patches", p("img"), p("lab"), erecs.ctypes.data_as(ctypes.POINTER(_lib.RsuElastic)), n, ext.shape[0], ext.shape[1], lab.shape[1], S, P,
         p("ex"), p("ey"), hu.stream())
    A.check("affine / elastic patches")
    torch.cuda.synchronize()
    np.testing.assert_array_equal(A["x"].cpu().numpy().view(np.int32), hx[:n].view(np.int32))
    np.testing.assert_array_equal(A["y"].cpu().numpy(), hy[:n])
    np.testing.assert_array_equal(A["ex"].cpu().numpy().view(np.int32), ehx[200:200 + n].view(np.int32))
    np.testing.assert_array_equal(A["ey"].cpu().numpy(), ehy[200:200 + n])
    assert (erecs["alpha"] > 0).any()


@pytest.mark.parametrize("S,nrec", [(11, 3), (37, 33)])
def test_color_jitter(S, nrec, placement="aligned"):
    """test_gpu_jitter.test_kernels_equal_the_host_mirror's launch: x in place, the workspace exactly rsu_color_jitter_ws_bytes"""
    from road_segmentation_unet_amd import _lib, hostio
    from tests import jitter_util as ju
    x = ju.make_batch(nrec, S, seed=100 * S + nrec)
    recs = np.ascontiguousarray(ju.mixed_records(nrec, seed=S + nrec))
    want = hostio.color_jitter(x, recs)
    nws = lib().rsu_color_jitter_ws_bytes(nrec, S)
    assert nws % 8 == 0 and (x.size * 4) % 512 != 0
    A = F.Arena(hu.DEV, [F.state("x", x), F.ws("ws", nws // 8, torch.int64)], placement=placement)
    call("rsu_color_jitter", hu.ptr(A["x"]), recs.ctypes.data_as(ctypes.POINTER(_lib.RsuJitter)), nrec, S, hu.ptr(A["ws"]), hu.stream())
    A.check("color_jitter S %d nrec %d" % (S, nrec))
    np.testing.assert_array_equal(_host(A["x"]), want)


# =========================================================================================== positive controls
def test_control_output_carved_one_row_short():
    """3x3 forward: y is carved one image row shorter than the call is told. Everything stays inside the arena (the row lands in the
    band); the fence must name y's `behind` side."""
    N, H, W, Cin, Cout, dil, _ = CONV[0]
    with pytest.raises(F.FenceError) as e:
        _conv_fwd(CONV[0], 1, y_rows_short=1, compare=False)
    row = (W - 2 * dil) * Cout * 2
    assert (e.value.tensor, e.value.side, e.value.first) == ("y", "behind", 0) and e.value.last < row and e.value.count > row // 2, str(e.value)


def test_control_workspace_carved_one_slab_short():
    """transposed-conv weight gradient at (4, 52, 50, 96 -> 96): 163 pixel tiles, so the launch uses all 128 slabs the size function
    advertises; the workspace is carved one slab short and the fence must name its `behind` side"""
    shape = (4, 52, 50, 96, 96, False)
    assert (shape[0] * shape[1] * shape[2] + 63) // 64 >= 128
    with pytest.raises(F.FenceError) as e:
        _convT(shape, ws_slabs_short=1, compare=False)
    assert (e.value.tensor, e.value.side, e.value.first) == ("ws", "behind", 0), str(e.value)


def test_control_last_input_row_is_band():
    """element-wise: the junction's skip gradient is carved one image row short, so its last row is band. Nothing is written out of place
    -- the fence passes -- but the pattern is read: dz = (pool gradient + skip gradient) * (y_act > 0) is NaN in that row wherever the
    activation is positive, and the comparison of dz must fail on NaN. (The pool's own input would not do: the hardware's max drops a
    NaN, and a NaN activation fails `> 0`.) The same for the 3x3 forward's input, without ReLU."""
    with pytest.raises(AssertionError, match="out of tolerance") as e:
        _pool_junction((2, 12, 16, 64), dskip_rows_short=1)
    assert not isinstance(e.value, F.FenceError) and "pool_skip_relu_bwd dz" in str(e.value) and ("(nan)" in str(e.value) or " got nan " in str(e.value)), str(e.value)
    with pytest.raises(AssertionError, match="out of tolerance") as e:
        _conv_fwd(CONV[0], 0, x_rows_short=1)      # (without ReLU: the hardware's max(NaN, 0) is 0 -- out of tolerance as well, but no NaN)
    assert not isinstance(e.value, F.FenceError) and "nan" in str(e.value).lower(), str(e.value)


# =========================================================================================== the registry (tests/test_fence_host.py)
HELPERS = {
    "test_conv2d_fwd": (_conv_fwd, _packed), "test_conv2d_fwd_every_forced_shape": (_conv_fwd,), "test_conv2d_fwd_ncu32": (_conv_fwd,),
    "test_conv2d_fwd_cropped_sources": (_packed,), "test_conv2d_fwd_k_split": (_packed,), "test_conv2d_fwd_pool": (_packed,),
    "test_conv2d_bwd_data": (_bwd_data, _packed), "test_conv2d_bwd_data_every_forced_shape": (_bwd_data,), "test_conv2d_bwd_data_ncu32": (_bwd_data,),
    "test_conv2d_bwd_data_k_split": (_bwd_data,), "test_conv2d_bwd_weight_and_bias_grad": (_wgrad,), "test_conv2d_bwd_weight_every_kernel": (_wgrad,),
    "test_conv2d_bwd_weight_ncu32": (_wgrad,), "test_conv2d_bwd_weight_cropped_source": (_wgrad,),
    "test_convT": (_convT, _packed), "test_convT_every_kernel": (_convT,), "test_convT_ncu32": (_convT,),
    "test_first_layer": (_first,), "test_first_layer_every_kernel": (_first,), "test_first_layer_ncu32": (_first,),
    "test_pool_and_junction": (_pool_junction,), "test_update_and_pack_tables": (_packed,),
    "test_control_output_carved_one_row_short": (_conv_fwd,), "test_control_workspace_carved_one_slab_short": (_convT,),
    "test_control_last_input_row_is_band": (_pool_junction, _conv_fwd),
}
_CONV_FWD = ["test_conv2d_fwd", "test_conv2d_fwd_every_forced_shape", "test_conv2d_fwd_ncu32", "test_conv2d_fwd_cropped_sources",
             "test_control_output_carved_one_row_short"]
_TABLES = ["test_update_and_pack_tables"]
_OPT = ["test_momentum_adam_ema_accumulate_norm"]
FENCED = {
    "rsu_pack_conv_fwd": ["test_conv2d_fwd", "test_update_and_pack_tables"], "rsu_pack_conv_bwd": ["test_conv2d_bwd_data", "test_update_and_pack_tables"],
    "rsu_pack_convT_fwd": ["test_convT", "test_update_and_pack_tables"], "rsu_pack_convT_bwd": ["test_convT", "test_update_and_pack_tables"],
    "rsu_pack_conv_first": ["test_first_layer", "test_update_and_pack_tables"], "rsu_pack_table_run": _TABLES,
    "rsu_color_adjust_fwd": ["test_first_layer"], "rsu_conv_first_fwd": ["test_first_layer", "test_first_layer_every_kernel", "test_first_layer_ncu32"],
    "rsu_color_conv_first_fwd": ["test_first_layer"], "rsu_conv_first_bwd_weight": ["test_first_layer", "test_first_layer_every_kernel", "test_first_layer_ncu32"],
    "rsu_color_adjust_bwd": ["test_first_layer"],
    "rsu_head_fwd": ["test_heads"], "rsu_head_fwd_bwd": ["test_heads"], "rsu_head_fwd_bwd_w": ["test_heads"], "rsu_head_dice_sums": ["test_heads"],
    "rsu_head_fwd_bwd_dice": ["test_heads"], "rsu_head_eval": ["test_heads"], "rsu_border_map": ["test_border_map"],
    "rsu_conv2d_fwd": _CONV_FWD, "rsu_conv2d_fwd_k": ["test_conv2d_fwd_k_split"], "rsu_conv2d_fwd_pool": ["test_conv2d_fwd_pool"],
    "rsu_conv2d_fwd_pool_k": ["test_conv2d_fwd_pool"],
    "rsu_conv2d_bwd_data": ["test_conv2d_bwd_data", "test_conv2d_bwd_data_every_forced_shape", "test_conv2d_bwd_data_ncu32", "test_conv2d_bwd_data_source_slice"],
    "rsu_conv2d_bwd_data_k": ["test_conv2d_bwd_data_k_split"],
    "rsu_conv2d_bwd_weight": ["test_conv2d_bwd_weight_and_bias_grad", "test_conv2d_bwd_weight_every_kernel", "test_conv2d_bwd_weight_ncu32",
                              "test_conv2d_bwd_weight_cropped_source"],
    "rsu_wgrad_group_run": ["test_wgrad_group"], "rsu_bias_grad": ["test_conv2d_bwd_weight_and_bias_grad"],
    "rsu_maxpool2x2_fwd": ["test_pool_and_junction"], "rsu_maxpool2x2_fwd_code": ["test_pool_and_junction"],
    "rsu_pool_skip_relu_bwd": ["test_pool_and_junction"], "rsu_pool_skip_relu_bwd_code": ["test_pool_and_junction"],
    "rsu_dropout_fwd": ["test_dropout_fwd", "test_convT"],
    "rsu_convT2x2_fwd": ["test_convT", "test_convT_every_kernel", "test_convT_ncu32"], "rsu_convT2x2_bwd_data": ["test_convT", "test_convT_every_kernel", "test_convT_ncu32"],
    "rsu_convT2x2_bwd_weight": ["test_convT", "test_convT_every_kernel", "test_convT_ncu32", "test_control_workspace_carved_one_slab_short"],
    "rsu_momentum_step": _OPT, "rsu_adam_step": _OPT, "rsu_grad_norm": _OPT + _TABLES, "rsu_ema_step": _OPT, "rsu_grad_accumulate": _OPT,
    "rsu_update_table_run": _TABLES, "rsu_update_table_run_adam": _TABLES, "rsu_update_table_run_clip": _TABLES, "rsu_update_table_run_adam_clip": _TABLES,
    "rsu_extract_tiles": ["test_tilers_square_and_rect"], "rsu_overlap_add": ["test_tilers_square_and_rect"], "rsu_overlap_finish": ["test_tilers_square_and_rect"],
    "rsu_extract_tiles_rect": ["test_tilers_square_and_rect"], "rsu_overlap_add_rect": ["test_tilers_square_and_rect"],
    "rsu_affine_patches": ["test_affine_and_elastic_patches"], "rsu_elastic_patches": ["test_affine_and_elastic_patches"],
    "rsu_color_jitter": ["test_color_jitter"], "rsu_quantize_mask": ["test_quantize_labels_confusion"],
    "rsu_quantize_mask_rect": ["test_quantize_labels_confusion"], "rsu_labels_for_patches": ["test_quantize_labels_confusion"],
    "rsu_confusion_counts": ["test_quantize_labels_confusion"],
}
NOT_FENCED = {}      # entry -> reason; only an entry that writes no device memory may stand here
SIZES = {
    "rsu_packed_bytes": ["test_conv2d_fwd", "test_conv2d_bwd_data", "test_convT", "test_update_and_pack_tables"],
    "rsu_packed_first_bytes": ["test_first_layer", "test_update_and_pack_tables"],
    "rsu_conv_first_bwd_ws_floats": ["test_first_layer"], "rsu_head_ws_floats": ["test_heads"], "rsu_head_w_ws_floats": ["test_heads"],
    "rsu_head_dice_ws_floats": ["test_heads"], "rsu_head_eval_ws_floats": ["test_heads"], "rsu_border_map_ws_bytes": ["test_border_map"],
    "rsu_conv_splitk_ws_floats": ["test_conv2d_fwd_k_split", "test_conv2d_bwd_data_k_split", "test_conv2d_fwd_pool"],
    "rsu_conv2d_bwd_weight_ws_floats": ["test_conv2d_bwd_weight_and_bias_grad"], "rsu_wgrad_group_ws_floats": ["test_wgrad_group"],
    "rsu_bias_grad_ws_floats": ["test_conv2d_bwd_weight_and_bias_grad"], "rsu_convT2x2_bwd_weight_ws_floats": ["test_convT"],
    "rsu_grad_norm_ws_floats": ["test_momentum_adam_ema_accumulate_norm", "test_update_and_pack_tables"], "rsu_color_jitter_ws_bytes": ["test_color_jitter"],
}
