"""-m gpu: every batch-taking launch of the training step and of prediction with its largest tensor just under the 2-GiB limit
(N = n_max of tests/large_util.LIMITS, the last image ends within one image of 0x7ffffff0 bytes), against the CPU oracle.

The kernels address a tensor through 32-bit byte offsets and form per-point offsets in int: whether every such product stays in range
shows only when the base sits just below 2^31. Two per-image geometries: "small" (66 x 66: N in the thousands, stresses products in n)
and "large" (260 x 258, not square, not a multiple of the tile sizes: N = 100..500, stresses products in rows and the overshoot of
partial last tiles). The batch is periodic over K = 3 images (tests/large_util.py): the reference is the oracle on those K images, the
comparison runs on the device over ALL images in chunks, with the op tolerances of tests/hiputil.py (no new tolerance). Weight
gradients, which sum over the batch, get a dz that is non-zero in eight images only -- the first, the last, the one that holds byte 2^30
of the input and its successor, four seeded others -- so the reference is the float64 sum of eight per-image oracle gradients and a
misaddressed read shows as a missing or foreign contribution. Outputs are pre-filled with NaN."""
import ctypes

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_oracle as U  # noqa: E402
from tests import hiputil as hu  # noqa: E402
from tests import large_util as lu  # noqa: E402
from road_segmentation_unet_amd._lib import RsuSrc, RsuWgradJob, call, lib  # noqa: E402

GEO = {"small": (66, 66), "large": (260, 258)}
K = lu.K


@pytest.fixture(autouse=True)
def _large_test():
    lu.need_memory()
    yield
    lu.done()


def _rand(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def _plan_lines(capfd):
    return [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("[plan fwd2]")]


def _eight(N, per_image_bytes, seed):
    """the eight images of a sparse gradient: first, last, the one holding byte 2^30 of the tensor and the next, four seeded others"""
    s = lu.straddler(per_image_bytes)
    assert 0 < s < s + 1 < N - 1 and s * per_image_bytes <= (1 << 30) < (s + 1) * per_image_bytes
    picks = [0, N - 1, s, s + 1]
    rng = np.random.RandomState(seed)
    while len(picks) < 8:
        n = int(rng.randint(1, N - 1))
        if n not in picks:
            picks.append(n)
    return picks


# ------------------------------------------------------------------------------------------- 3x3 conv forward
CONV_FWD = [
    # geometry, Cin, Cout, dil, RSU_FWD_GEN (None: the default)
    ("small", 64, 64, 1, None),    # the input at the limit
    ("large", 64, 64, 1, None),
    ("small", 32, 64, 1, None),    # the output at the limit
    ("large", 32, 64, 1, None),
    ("small", 64, 64, 2, None),    # dilation 2
    ("large", 64, 64, 2, None),
    ("large", 64, 64, 1, "2"),     # both kernel generations at the planner's own shape
    ("large", 64, 64, 1, "4"),
]


@pytest.mark.parametrize("geo,Cin,Cout,dil,gen", CONV_FWD)
def test_conv2d_fwd_at_the_limit(geo, Cin, Cout, dil, gen, monkeypatch):
    if gen:
        monkeypatch.setenv("RSU_FWD_GEN", gen)
    H, W = GEO[geo]
    N = lu.entry_n_max("rsu_conv2d_fwd", H, W, Cin, Cout, dil)
    rng = np.random.RandomState(Cin + Cout + dil + H)
    base = lu.base_images(Cin * 3 + H, (H, W, Cin))
    w = _rand(rng, 3, 3, Cin, Cout, scale=1.0 / np.sqrt(9 * Cin))
    b = _rand(rng, Cout, scale=0.1)
    ref = U.conv2d_fwd(base, hu.q(w), b, dil=dil, relu=True)
    xd, wp, bd = lu.periodic(base, N), hu.pack_conv_fwd(w), hu.dev_f32(b)
    y = lu.nan_out((N, H - 2 * dil, W - 2 * dil, Cout))
    s = (RsuSrc * 1)(hu.src_of(xd, H, W))
    call("rsu_conv2d_fwd", s, 1, hu.ptr(wp), hu.ptr(bd), hu.ptr(y), N, H, W, Cout, dil, 1, 0, hu.stream())
    lu.assert_bf16_periodic(y, ref, "conv2d_fwd %s %d->%d dil %d gen %s N %d" % (geo, Cin, Cout, dil, gen, N))
    lu.assert_periodic_bits(y, "conv2d_fwd")   # (no split-K at these sizes: the summation order of a pixel does not depend on its tile)


@pytest.mark.parametrize("geo", ["small", "large"])
def test_conv2d_fwd_two_cropped_sources_at_the_limit(geo):
    """the virtual crop + concat of a decoder conv: the skip tensor, 24 pixels larger than the window, is the tensor at the limit"""
    h, w = GEO[geo]
    Ha, Wa, C, Cout = h + 24, w + 24, 32, 32
    N = lu.n_max(Ha * Wa * C * 2)
    assert N * (h - 2) * (w - 2) * Cout * 2 < lu.LIMIT
    rng = np.random.RandomState(h)
    a, c = lu.base_images(h + 1, (Ha, Wa, C)), lu.base_images(h + 2, (h, w, C))
    Wt = _rand(rng, 3, 3, 2 * C, Cout, scale=1.0 / np.sqrt(18 * C))
    b = _rand(rng, Cout, scale=0.1)
    ref = U.conv2d_fwd(np.concatenate([U.center_crop(a, h, w), c], axis=3), hu.q(Wt), b, relu=True)
    ad, cd, wp, bd = lu.periodic(a, N), lu.periodic(c, N), hu.pack_conv_fwd(Wt, [C, C]), hu.dev_f32(b)
    y = lu.nan_out((N, h - 2, w - 2, Cout))
    srcs = (RsuSrc * 2)(hu.src_of(ad, h, w), hu.src_of(cd, h, w))
    call("rsu_conv2d_fwd", srcs, 2, hu.ptr(wp), hu.ptr(bd), hu.ptr(y), N, h, w, Cout, 1, 1, 0, hu.stream())
    lu.assert_bf16_periodic(y, ref, "conv2d_fwd two cropped sources %s N %d" % (geo, N))
    lu.assert_periodic_bits(y, "conv2d_fwd two sources")


def _code_of(x):
    """rsu_maxpool2x2_fwd_code's code bytes of x [n][H][W][C] (H, W even): bits 0-3 = (window element 2 dy + dx > 0), bits 4-5 = the
    window's first maximum in row-major order"""
    e = [x[:, dy::2, dx::2, :] for dy in (0, 1) for dx in (0, 1)]
    best = np.zeros(e[0].shape, np.uint8)
    m = e[0].copy()
    for k in (1, 2, 3):
        up = e[k] > m
        best[up] = k
        m = np.where(up, e[k], m)
    code = best << 4
    for k in range(4):
        code |= (e[k] > 0).astype(np.uint8) << k
    return code.astype(np.uint8)


@pytest.mark.parametrize("geo", ["small", "large"])
def test_conv2d_fwd_pool_with_code_at_the_limit(geo):
    H, W = GEO[geo]
    Cin = Cout = 64
    N = lu.entry_n_max("rsu_conv2d_fwd_pool", H, W, Cin, Cout)
    rng = np.random.RandomState(H + 5)
    base = lu.base_images(H + 6, (H, W, Cin))
    w = _rand(rng, 3, 3, Cin, Cout, scale=1.0 / np.sqrt(9 * Cin))
    b = _rand(rng, Cout, scale=0.1)
    ref = U.conv2d_fwd(base, hu.q(w), b, relu=True)
    xd, wp, bd = lu.periodic(base, N), hu.pack_conv_fwd(w), hu.dev_f32(b)
    Ho, Wo = H - 2, W - 2
    y, pooled = lu.nan_out((N, Ho, Wo, Cout)), lu.nan_out((N, Ho // 2, Wo // 2, Cout))
    code = torch.full((N, Ho // 2, Wo // 2, Cout), 0xAA, dtype=torch.uint8, device=hu.DEV)
    s = (RsuSrc * 1)(hu.src_of(xd, H, W))
    call("rsu_conv2d_fwd_pool", s, 1, hu.ptr(wp), hu.ptr(bd), hu.ptr(y), hu.ptr(pooled), hu.ptr(code), N, H, W, Cout, 1.0, 0, 0, hu.stream())
    lu.assert_bf16_periodic(y, ref, "conv2d_fwd_pool activation %s N %d" % (geo, N))
    lu.assert_bf16_periodic(pooled, U.maxpool_fwd(hu.q(ref)), "conv2d_fwd_pool pooled %s" % geo)
    # the code bytes are a function of the activation: those of the first K images from the (checked) activation, every other image by bits
    y_k = hu.host(y[:K])
    assert np.array_equal(code[:K].cpu().numpy(), _code_of(y_k)), "code bytes of the first images"
    assert np.array_equal(hu.host(pooled[:K]), U.maxpool_fwd(y_k)), "pooled is the maximum of the stored activation"
    for t, what in ((y, "activation"), (pooled, "pooled"), (code, "code bytes")):
        lu.assert_periodic_bits(t, "conv2d_fwd_pool " + what)


# ------------------------------------------------------------------------------------------- 3x3 conv backward data
BWD_DATA = [
    # geometry, Cin_total, ci_off, ci_cnt, Cout, dil, mode
    ("small", 64, 0, 64, 64, 1, "mask"),
    ("large", 64, 0, 64, 64, 1, "mask"),
    ("small", 64, 0, 64, 64, 2, "accumulate"),
    ("large", 64, 0, 64, 64, 2, "accumulate"),
    ("large", 96, 32, 32, 64, 1, "slice"),     # towards one concat source: dz, the larger tensor, at the limit
]


@pytest.mark.parametrize("geo,Cin_total,ci_off,ci_cnt,Cout,dil,mode", BWD_DATA)
def test_conv2d_bwd_data_at_the_limit(geo, Cin_total, ci_off, ci_cnt, Cout, dil, mode):
    H, W = GEO[geo]
    Hd, Wd = H - 2 * dil, W - 2 * dil
    N = lu.n_max(max(H * W * ci_cnt * 2, Hd * Wd * Cout * 2))
    rng = np.random.RandomState(H + Cout + dil + ci_off)
    dz = lu.base_images(H + dil, (Hd, Wd, Cout))
    w = _rand(rng, 3, 3, Cin_total, Cout, scale=1.0 / np.sqrt(9 * Cout))
    g = U.conv2d_bwd_data(dz, hu.q(w), (H, W), dil=dil)[..., ci_off:ci_off + ci_cnt]
    dzd = lu.periodic(dz, N)
    wp = hu.pack_conv_bwd(w, ci_off, ci_cnt) if mode == "slice" else hu.pack_conv_bwd(w)
    what = "conv2d_bwd_data %s %s dil %d N %d" % (mode, geo, dil, N)
    if mode == "mask":
        yprev = lu.base_images(H + 9, (H, W, ci_cnt), relu=True)
        yd = lu.periodic(yprev, N)
        dx = lu.nan_out((N, H, W, ci_cnt))
        call("rsu_conv2d_bwd_data", hu.ptr(dzd), hu.ptr(wp), hu.ptr(dx), hu.ptr(yd), 0, N, H, W, Cin_total, 0, ci_cnt, Cout, dil, 0, hu.stream())
        lu.assert_bf16_periodic(dx, U.relu_bwd(yprev, g), what)
    elif mode == "accumulate":   # dx += result: q(stored + sum), one rounding of an fp32 value
        d0 = lu.base_images(H + 11, (H, W, ci_cnt))
        dx = lu.periodic(d0, N)
        call("rsu_conv2d_bwd_data", hu.ptr(dzd), hu.ptr(wp), hu.ptr(dx), None, 1, N, H, W, Cin_total, 0, ci_cnt, Cout, dil, 0, hu.stream())
        lu.assert_bf16_periodic(dx, (d0.astype(np.float64) + g).astype(np.float32), what)
    else:
        dx = lu.nan_out((N, H, W, ci_cnt))
        call("rsu_conv2d_bwd_data", hu.ptr(dzd), hu.ptr(wp), hu.ptr(dx), None, 0, N, H, W, ci_cnt, 0, ci_cnt, Cout, 1, 0, hu.stream())
        lu.assert_bf16_periodic(dx, g, what)
    lu.assert_periodic_bits(dx, what)


# ------------------------------------------------------------------------------------------- 3x3 conv backward weight
@pytest.mark.parametrize("geo", ["small", "large"])
def test_conv2d_bwd_weight_and_group_at_the_limit(geo):
    """rsu_conv2d_bwd_weight (default plan) and rsu_wgrad_group_run on one job: x periodic and at the limit, dz non-zero in eight images"""
    H, W = GEO[geo]
    Cin = Cout = 64
    Ho, Wo = H - 2, W - 2
    N = lu.entry_n_max("rsu_conv2d_bwd_weight", H, W, Cin, Cout)
    x = lu.base_images(H + 21, (H, W, Cin))
    picks = _eight(N, H * W * Cin * 2, H)
    rng = np.random.RandomState(H + 22)
    dzs = {n: hu.q(_rand(rng, Ho, Wo, Cout, scale=0.1)) for n in picks}
    ref_dw, ref_db = np.zeros((3, 3, Cin, Cout), np.float64), np.zeros(Cout, np.float64)
    for n in picks:
        dw_n, db_n = U.conv2d_bwd_weight(x[n % K][None], dzs[n][None])
        ref_dw += dw_n
        ref_db += db_n
    xd, dzd = lu.periodic(x, N), lu.sparse(dzs, N, (Ho, Wo, Cout))
    dw, db = lu.nan_out((3, 3, Cin, Cout), torch.float32), lu.nan_out((Cout,), torch.float32)
    nws = lib().rsu_conv2d_bwd_weight_ws_floats(Cin, Cin, Cout)
    ws = torch.zeros(nws + 4096, dtype=torch.float32, device=hu.DEV)
    ws[nws:] = 12345.0
    s = hu.src_of(xd, H, W)
    call("rsu_conv2d_bwd_weight", ctypes.byref(s), hu.ptr(dzd), hu.ptr(dw), hu.ptr(db), hu.ptr(ws), N, Ho, Wo, Cin, 0, Cout, 1, 0, hu.stream())
    hu.assert_f32_close(hu.host(dw), ref_dw, "conv2d_bwd_weight %s N %d images %s" % (geo, N, picks))
    hu.assert_f32_close(hu.host(db), ref_db, "conv2d_bwd_weight bias %s" % geo)
    assert bool((ws[nws:] == 12345.0).all()), "workspace overrun"
    # the grouped launch on the same job
    gdw, gdb = lu.nan_out((3, 3, Cin, Cout), torch.float32), lu.nan_out((Cout,), torch.float32)
    jobs = (RsuWgradJob * 1)(RsuWgradJob(0, hu.src_of(xd, H, W), dzd.data_ptr(), gdw.data_ptr(), gdb.data_ptr(), Ho, Wo, Cin, 0, Cout, 1))
    gws = torch.zeros(lib().rsu_wgrad_group_ws_floats(), dtype=torch.float32, device=hu.DEV)
    table = ctypes.create_string_buffer(lib().rsu_wgrad_group_table_bytes())
    assert lib().rsu_wgrad_group_plan(jobs, 1, hu.ptr(gws), N, 0, table) == 0
    devt = torch.frombuffer(bytearray(table.raw), dtype=torch.uint8).to(hu.DEV)
    call("rsu_wgrad_group_run", table, hu.ptr(devt), hu.stream())
    hu.assert_f32_close(hu.host(gdw), ref_dw, "wgrad group %s N %d" % (geo, N))
    hu.assert_f32_close(hu.host(gdb), ref_db, "wgrad group bias %s" % geo)
    lu.note("conv2d_bwd_weight %s N %d, dz in images %s" % (geo, N, picks), N, N * H * W * Cin * 2, hu.host(dw), ref_dw)
    lu.note("wgrad group, one job %s N %d" % (geo, N), N, N * H * W * Cin * 2, hu.host(gdw), ref_dw)


# ------------------------------------------------------------------------------------------- transposed conv
CONVT = [
    # geometry of the OUTPUT (the input is half of it), Cin, Cout
    ("small", 64, 32),     # the 4x output at the limit
    ("large", 64, 32),
    ("small", 256, 32),    # the input at the limit (Cin > 4 Cout)
]


@pytest.mark.parametrize("geo,Cin,Cout", CONVT)
def test_convT_at_the_limit(geo, Cin, Cout, capfd, monkeypatch):
    """rsu_convT2x2_fwd / _bwd_data / _bwd_weight; the forward and backward-data launches are igemm_ct's (no [plan fwd2] line). The
    pixel-count branch of igemm_wgt / igemm_wg1 (2^28 pixels) cannot be reached below the byte limit: tests/test_large_limits_host.py"""
    monkeypatch.setenv("RSU_PLAN_DEBUG", "1")
    H, W = GEO[geo][0] // 2, GEO[geo][1] // 2
    N = lu.entry_n_max("rsu_convT2x2_fwd", H, W, Cin, Cout)
    assert N * H * W < 1 << 24   # igemm_ct's own bound
    rng = np.random.RandomState(Cin + H)
    x = lu.base_images(H + 31, (H, W, Cin), relu=True)
    Kt = _rand(rng, 2, 2, Cout, Cin, scale=1.0 / np.sqrt(Cin))
    b = _rand(rng, Cout, scale=0.1)
    seg, seg2 = (ctypes.c_int * 1)(Cin), (ctypes.c_int * 1)(Cout)
    pf = torch.zeros(4 * lib().rsu_packed_bytes(1, Cout, seg, 1) // 2, dtype=torch.bfloat16, device=hu.DEV)
    pb = torch.zeros(lib().rsu_packed_bytes(4, Cin, seg2, 1) // 2, dtype=torch.bfloat16, device=hu.DEV)
    Kd, bd = hu.dev_f32(Kt), hu.dev_f32(b)
    call("rsu_pack_convT_fwd", hu.ptr(Kd), hu.ptr(pf), Cin, Cout, hu.stream())
    call("rsu_pack_convT_bwd", hu.ptr(Kd), hu.ptr(pb), Cin, Cout, hu.stream())
    xd = lu.periodic(x, N)
    y = lu.nan_out((N, 2 * H, 2 * W, Cout))
    capfd.readouterr()
    call("rsu_convT2x2_fwd", hu.ptr(xd), hu.ptr(pf), hu.ptr(bd), hu.ptr(y), N, H, W, Cin, Cout, 0, hu.stream())
    assert not _plan_lines(capfd), "the forward launch left igemm_ct"
    lu.assert_bf16_periodic(y, U.convT_fwd(x, hu.q(Kt), b), "convT fwd %s %d->%d N %d" % (geo, Cin, Cout, N))
    lu.assert_periodic_bits(y, "convT fwd")
    del y
    dy = lu.base_images(H + 32, (2 * H, 2 * W, Cout), scale=0.1)
    dyd = lu.periodic(dy, N)
    dx = lu.nan_out((N, H, W, Cin))
    capfd.readouterr()
    call("rsu_convT2x2_bwd_data", hu.ptr(dyd), hu.ptr(pb), hu.ptr(dx), hu.ptr(xd), 1.0, N, H, W, Cin, Cout, 0, hu.stream())
    assert not _plan_lines(capfd), "the backward-data launch left igemm_ct"
    rdx = U.convT_bwd(x, hu.q(Kt), dy)[0]
    lu.assert_bf16_periodic(dx, U.relu_bwd(x, rdx), "convT bwd_data %s %d->%d N %d" % (geo, Cin, Cout, N))
    lu.assert_periodic_bits(dx, "convT bwd_data")
    del dx, dyd
    # weight gradient: dy non-zero in eight images
    picks = _eight(N, max(lu.LIMITS["rsu_convT2x2_bwd_weight"](H, W, Cin, Cout)), H + Cin)
    dys = {n: hu.q(_rand(rng, 2 * H, 2 * W, Cout, scale=0.1)) for n in picks}
    ref_dK, ref_db = np.zeros((2, 2, Cout, Cin), np.float64), np.zeros(Cout, np.float64)
    for n in picks:
        _, dK_n, db_n = U.convT_bwd(x[n % K][None], np.zeros((2, 2, Cout, Cin), np.float32), dys[n][None], need_dx=False)
        ref_dK += dK_n
        ref_db += db_n
    dysd = lu.sparse(dys, N, (2 * H, 2 * W, Cout))
    dK, dbT = lu.nan_out((2, 2, Cout, Cin), torch.float32), lu.nan_out((Cout,), torch.float32)
    nws = lib().rsu_convT2x2_bwd_weight_ws_floats(Cin, Cout)
    ws = torch.zeros(nws + 4096, dtype=torch.float32, device=hu.DEV)
    ws[nws:] = 12345.0
    call("rsu_convT2x2_bwd_weight", hu.ptr(xd), hu.ptr(dysd), hu.ptr(dK), hu.ptr(dbT), hu.ptr(ws), N, H, W, Cin, Cout, 0, hu.stream())
    assert bool((ws[nws:] == 12345.0).all()), "workspace overrun"
    hu.assert_f32_close(hu.host(dK), ref_dK, "convT bwd_weight %s %d->%d N %d images %s" % (geo, Cin, Cout, N, picks))
    hu.assert_f32_close(hu.host(dbT), ref_db, "convT bias grad %s" % geo)
    lu.note("convT bwd_weight %s %d->%d N %d, dy in images %s" % (geo, Cin, Cout, N, picks), N,
            N * max(lu.LIMITS["rsu_convT2x2_bwd_weight"](H, W, Cin, Cout)), hu.host(dK), ref_dK)


# ------------------------------------------------------------------------------------------- first layer
@pytest.mark.parametrize("geo,Cout", [("small", 64), ("large", 64), ("small", 8), ("large", 8)])
def test_first_conv_at_the_limit(geo, Cout):
    """rsu_conv_first_fwd and rsu_conv_first_bwd_weight: Cout = 64 puts the output (128 bytes per pixel) at the limit, Cout = 8 the
    16-channel input tensor (32 bytes per pixel)"""
    H, W = GEO[geo]
    Ho, Wo = H - 2, W - 2
    N = lu.entry_n_max("rsu_conv_first_fwd", H, W, Cout)
    rng = np.random.RandomState(H + Cout)
    in16 = lu.base_images(H + Cout + 1, (H, W, 16))
    w1, b1 = _rand(rng, 3, 3, 3, Cout, scale=0.3), _rand(rng, Cout, scale=0.1)
    ind, w1d, b1d = lu.periodic(in16, N), hu.dev_f32(w1), hu.dev_f32(b1)
    pk1 = torch.zeros(lib().rsu_packed_first_bytes(Cout) // 2, dtype=torch.bfloat16, device=hu.DEV)
    call("rsu_pack_conv_first", hu.ptr(w1d), hu.ptr(pk1), Cout, hu.stream())
    y = lu.nan_out((N, Ho, Wo, Cout))
    call("rsu_conv_first_fwd", hu.ptr(ind), hu.ptr(pk1), hu.ptr(b1d), hu.ptr(y), N, H, W, Cout, 1, 0, hu.stream())
    lu.assert_bf16_periodic(y, U.conv2d_fwd(in16[..., 0:3], hu.q(w1), b1), "conv_first_fwd %s Cout %d N %d" % (geo, Cout, N))
    lu.assert_periodic_bits(y, "conv_first_fwd")
    del y
    picks = _eight(N, max(lu.LIMITS["rsu_conv_first_bwd_weight"](H, W, Cout)), H + Cout)
    dzs = {n: hu.q(_rand(rng, Ho, Wo, Cout, scale=0.1)) for n in picks}
    ref = np.zeros((3, 3, 16, Cout), np.float64)
    ref_db = np.zeros(Cout, np.float64)
    for n in picks:
        ref += U.conv2d_bwd_weight(in16[n % K][None], dzs[n][None])[0]
        ref_db += dzs[n].reshape(-1, Cout).astype(np.float64).sum(0)
    dzd = lu.sparse(dzs, N, (Ho, Wo, Cout))
    dw1, gx = lu.nan_out((3, 3, 3, Cout), torch.float32), lu.nan_out((9, 12, Cout), torch.float32)
    db = lu.nan_out((Cout,), torch.float32)
    ws = torch.zeros(lib().rsu_conv_first_bwd_ws_floats(Cout), dtype=torch.float32, device=hu.DEV)
    call("rsu_conv_first_bwd_weight", hu.ptr(ind), hu.ptr(dzd), hu.ptr(dw1), hu.ptr(gx), hu.ptr(db), hu.ptr(ws), N, H, W, Cout, 1, 0, hu.stream())
    hu.assert_f32_close(hu.host(dw1), ref[:, :, 0:3], "conv_first dW %s Cout %d N %d images %s" % (geo, Cout, N, picks))
    hu.assert_f32_close(hu.host(gx), ref[:, :, 4:16].reshape(9, 12, Cout), "conv_first gx %s" % geo)
    hu.assert_f32_close(hu.host(db), ref_db, "conv_first db %s" % geo)
    lu.note("conv_first_bwd_weight %s Cout %d N %d, dz in images %s" % (geo, Cout, N, picks), N,
            N * max(lu.LIMITS["rsu_conv_first_bwd_weight"](H, W, Cout)), hu.host(gx), ref[:, :, 4:16].reshape(9, 12, Cout))


@pytest.mark.parametrize("geo", ["small", "large"])
def test_colour_adjust_fused_first_conv_at_the_limit(geo):
    """rsu_color_conv_first_fwd from the f32 input: the output (Cout = 64) at the limit -- the input, 12 bytes per pixel, cannot be (the
    fewest output channels, 8, are 16 bytes per pixel). The reference is the oracle's conv on the device's own bf16 net0 of the K images
    (as tests/test_gpu_ops.py does: a 1-ulp flip of net0 is not this kernel's)"""
    H, W = GEO[geo]
    Cout = 64
    N = lu.entry_n_max("rsu_color_conv_first_fwd", H, W, Cout)
    rng = np.random.RandomState(H + 41)
    x = rng.rand(K, H, W, 3).astype(np.float32)
    w0, b0 = _rand(rng, 3, 3, scale=0.5), _rand(rng, 3, scale=0.1)
    w1, b1 = _rand(rng, 3, 3, 3, Cout, scale=0.3), _rand(rng, Cout, scale=0.1)
    xd, w0d, b0d, w1d, b1d = lu.periodic(x, N, torch.float32), hu.dev_f32(w0), hu.dev_f32(b0), hu.dev_f32(w1), hu.dev_f32(b1)
    pk1 = torch.zeros(lib().rsu_packed_first_bytes(Cout) // 2, dtype=torch.bfloat16, device=hu.DEV)
    call("rsu_pack_conv_first", hu.ptr(w1d), hu.ptr(pk1), Cout, hu.stream())
    in16 = lu.nan_out((K, H, W, 16))
    call("rsu_color_adjust_fwd", hu.ptr(xd), hu.ptr(w0d), hu.ptr(b0d), hu.ptr(in16), K * H * W, 1.0, 0, hu.stream())
    net0 = hu.host(in16)[..., 0:3]
    hu.assert_bf16_close(net0, U.conv1x1_fwd(x, w0, b0, sub=0.5), "color_adjust net0")
    y = lu.nan_out((N, H - 2, W - 2, Cout))
    call("rsu_color_conv_first_fwd", hu.ptr(xd), hu.ptr(w0d), hu.ptr(b0d), hu.ptr(pk1), hu.ptr(b1d), hu.ptr(y), N, H, W, Cout, 1, 0, hu.stream())
    lu.assert_bf16_periodic(y, U.conv2d_fwd(net0, hu.q(w1), b1), "color_conv_first_fwd %s N %d" % (geo, N))
    lu.assert_periodic_bits(y, "color_conv_first_fwd")


# ------------------------------------------------------------------------------------------- pool and gradient junction
@pytest.mark.parametrize("geo", ["small", "large"])
def test_maxpool_code_and_junction_at_the_limit(geo):
    """rsu_maxpool2x2_fwd_code and rsu_pool_skip_relu_bwd_code with the unpooled tensor at the limit"""
    H, W = GEO[geo]
    C = 64
    N = lu.entry_n_max("rsu_maxpool2x2_fwd_code", H, W, C)
    x = lu.base_images(H + 51, (H, W, C), relu=True)
    x[0, :4, :4, :] = x[0, 0, 0, :]   # ties (zeros included) in a corner
    xd = lu.periodic(x, N)
    y = lu.nan_out((N, H // 2, W // 2, C))
    code = torch.full((N, H // 2, W // 2, C), 0xAA, dtype=torch.uint8, device=hu.DEV)
    call("rsu_maxpool2x2_fwd_code", hu.ptr(xd), hu.ptr(y), hu.ptr(code), N, H, W, C, 1.0, 0, hu.stream())
    lu.assert_bf16_periodic(y, U.maxpool_fwd(x), "maxpool2x2_fwd_code %s N %d" % (geo, N))
    assert np.array_equal(hu.host(y[:K]), U.maxpool_fwd(x)) and np.array_equal(code[:K].cpu().numpy(), _code_of(x))   # exact: a maximum rounds nothing
    lu.assert_periodic_bits(y, "maxpool pooled")
    lu.assert_periodic_bits(code, "maxpool code bytes")
    del xd, y
    Hs, Ws = H - 8, W - 12
    dpool, dskip = lu.base_images(H + 52, (H // 2, W // 2, C)), lu.base_images(H + 53, (Hs, Ws, C))
    dpd, dsd = lu.periodic(dpool, N), lu.periodic(dskip, N)
    dz = lu.nan_out((N, H, W, C))
    call("rsu_pool_skip_relu_bwd_code", None, hu.ptr(code), hu.ptr(dpd), hu.ptr(dsd), hu.ptr(dz), N, H, W, C, Hs, Ws, 1.0, 0, hu.stream())
    ref = U.relu_bwd(x, U.maxpool_bwd(x, dpool) + U.center_pad_like(dskip, x.shape))
    lu.assert_bf16_periodic(dz, ref, "pool_skip_relu_bwd_code %s N %d" % (geo, N))
    lu.assert_periodic_bits(dz, "pool_skip_relu_bwd_code")


@pytest.mark.parametrize("geo", ["small", "large"])
def test_general_junction_odd_height_at_the_limit(geo):
    """rsu_pool_skip_relu_bwd from the activation, odd H (a last row outside every pooling window)"""
    H, W = GEO[geo][0] + 1, GEO[geo][1]
    C = 64
    N = lu.entry_n_max("rsu_pool_skip_relu_bwd", H, W, C)
    x = lu.base_images(H + 61, (H, W, C), relu=True)
    Hs, Ws = H - 7, W - 12
    dpool, dskip = lu.base_images(H + 62, (H // 2, W // 2, C)), lu.base_images(H + 63, (Hs, Ws, C))
    xd, dpd, dsd = lu.periodic(x, N), lu.periodic(dpool, N), lu.periodic(dskip, N)
    dz = lu.nan_out((N, H, W, C))
    call("rsu_pool_skip_relu_bwd", hu.ptr(xd), hu.ptr(dpd), hu.ptr(dsd), hu.ptr(dz), N, H, W, C, Hs, Ws, 1.0, 0, hu.stream())
    g = U.center_pad_like(dskip, x.shape)
    g[:, :H // 2 * 2, :W // 2 * 2] += U.maxpool_bwd(x[:, :H // 2 * 2, :W // 2 * 2], dpool)
    lu.assert_bf16_periodic(dz, U.relu_bwd(x, g), "pool_skip_relu_bwd odd H %s N %d" % (geo, N))
    lu.assert_periodic_bits(dz, "pool_skip_relu_bwd")


# ------------------------------------------------------------------------------------------- dropout
def _kept_fraction_ok(frac, n, keep):
    return abs(frac - keep) <= 6.0 * np.sqrt(keep * (1.0 - keep) / n)   # six standard deviations of a mean of n Bernoulli draws


def _either(out, a, b, what, keep, count_mask=None):
    """every element of out (bf16 [N, ...]) is within the bf16 op tolerance of a[n % K] (its dropout draw kept it) or of b[n % K]
    (dropped), and where the two differ the kept share of every chunk is `keep` (six standard deviations of n Bernoulli draws)"""
    qa, qb = (torch.from_numpy(hu.q(t)).to(hu.DEV) for t in (a, b))
    tol = lambda r: lu.BF16_ULPS * hu.BF16_ULP * r.abs() + lu.BF16_ATOL_SCALE * max(float(r.abs().max().item()), 1e-30)   # noqa: E731
    ta, tb = tol(qa), tol(qb)
    differ = (qa - qb).abs() > ta + tb
    for n0, c in lu._chunks(out):
        got = out[n0:n0 + c].to(torch.float32)
        if c % K == 0:
            got = got.view((c // K, K) + tuple(qa.shape[1:]))
            ea, eb, df = (got - qa).abs() <= ta, (got - qb).abs() <= tb, differ.unsqueeze(0).expand(got.shape)
        else:
            ea, eb, df = (got - qa[:c]).abs() <= ta[:c], (got - qb[:c]).abs() <= tb[:c], differ[:c]
        assert bool((ea | eb).all().item()), "%s: images %d..%d hold an element that is neither its kept nor its dropped value" % (what, n0, n0 + c - 1)
        n = int(df.sum().item())
        frac = float((ea & df).sum().item()) / n
        assert _kept_fraction_ok(frac, n, keep), (what, n0, c, frac)


@pytest.mark.parametrize("geo", ["small", "large"])
def test_maxpool_and_junction_with_dropout_at_the_limit(geo):
    """rsu_maxpool2x2_fwd_code and rsu_pool_skip_relu_bwd_code at keep 0.8: the mask is a hash of the GLOBAL pooled element index, so the
    outputs are not periodic. The first, the last and the image that holds byte 2^30 of the unpooled tensor against the oracle's mask on
    the host; every element of every other image is its kept or its dropped value, and the kept share of every chunk is keep"""
    H, W = GEO[geo]
    C, keep, key = 64, 0.8, 0x1234ABCD
    N = lu.entry_n_max("rsu_maxpool2x2_fwd_code", H, W, C)
    per = (H // 2) * (W // 2) * C
    inv = np.float32(1) / np.float32(keep)
    x = lu.base_images(H + 51, (H, W, C), relu=True)
    xd = lu.periodic(x, N)
    y = lu.nan_out((N, H // 2, W // 2, C))
    code = torch.full((N, H // 2, W // 2, C), 0xAA, dtype=torch.uint8, device=hu.DEV)
    call("rsu_maxpool2x2_fwd_code", hu.ptr(xd), hu.ptr(y), hu.ptr(code), N, H, W, C, keep, key, hu.stream())
    pooled = U.maxpool_fwd(x)
    three = (0, lu.straddler(H * W * C * 2), N - 1)
    masks = {n: lu.mask_range(n * per, per, keep, key).reshape(H // 2, W // 2, C) for n in three}
    for n in three:
        assert np.array_equal(hu.host(y[n]), hu.q(pooled[n % K] * masks[n] * inv)), "pooled image %d" % n
    _either(y, pooled * inv, np.zeros_like(pooled), "maxpool with dropout %s" % geo, keep)
    lu.assert_periodic_bits(code, "code bytes (no dropout in them)")
    assert np.array_equal(code[:K].cpu().numpy(), _code_of(x))
    del xd, y
    Hs, Ws = H - 8, W - 12
    dpool, dskip = lu.base_images(H + 52, (H // 2, W // 2, C)), lu.base_images(H + 53, (Hs, Ws, C))
    dpd, dsd = lu.periodic(dpool, N), lu.periodic(dskip, N)
    dz = lu.nan_out((N, H, W, C))
    call("rsu_pool_skip_relu_bwd_code", None, hu.ptr(code), hu.ptr(dpd), hu.ptr(dsd), hu.ptr(dz), N, H, W, C, Hs, Ws, keep, key, hu.stream())
    pad = U.center_pad_like(dskip, x.shape)
    for n in three:
        k = n % K
        ref = U.relu_bwd(x[k:k + 1], U.maxpool_bwd(x[k:k + 1], (dpool[k] * masks[n] * inv)[None]) + pad[k:k + 1])
        hu.assert_bf16_close(hu.host(dz[n])[None], ref, "junction with dropout, image %d" % n)
    _either(dz, U.relu_bwd(x, U.maxpool_bwd(x, dpool * inv) + pad), U.relu_bwd(x, pad), "junction with dropout %s" % geo, keep)
    lu.RECORD.append(dict(what="maxpool + junction keep 0.8 %s N %d" % (geo, N), N=N, bytes=N * H * W * C * 2, worst_err=0.0, scale=0.0))


@pytest.mark.parametrize("geo", ["small", "large"])
def test_dropout_fwd_at_the_limit(geo):
    """rsu_dropout_fwd at keep 0.8: the mask is a hash of the GLOBAL element index (up to 2^30 here), so the output is not periodic. The
    first, the last and the 2^30-straddling image against the oracle's mask on the host, bit for bit; every element of every image is
    either zero (dropped) or q(x / keep) of its periodic source; the kept fraction of every chunk is keep"""
    H, W = GEO[geo]
    C, keep, key = 64, 0.8, 0x5EED0001
    per = H * W * C
    N = lu.entry_n_max("rsu_dropout_fwd", H, W, C)
    x = lu.base_images(H + 71, (H, W, C))
    x[x == 0] = 1.0
    inv = np.float32(1) / np.float32(keep)
    xd = lu.periodic(x, N)
    y = lu.nan_out((N, H, W, C))
    call("rsu_dropout_fwd", hu.ptr(xd), hu.ptr(y), N * per, keep, key, hu.stream())
    for n in (0, lu.straddler(per * 2), N - 1):
        m = lu.mask_range(n * per, per, keep, key).reshape(H, W, C)
        assert np.array_equal(hu.host(y[n]), hu.q(x[n % K] * m * inv)), "image %d" % n
    full = torch.from_numpy(hu.q(x * inv)).to(hu.DEV).to(torch.bfloat16)
    for n0, c in lu._chunks(y):
        got = y[n0:n0 + c]
        src = full.unsqueeze(0).expand((c // K, K) + tuple(full.shape[1:])).reshape(got.shape) if c % K == 0 else full[:c]
        kept = got == src
        dropped = got == 0   # (a dropped negative element is -0: x * 0)
        assert bool((kept | dropped).all().item()), "images %d..%d: an element is neither dropped nor its scaled source" % (n0, n0 + c - 1)
        frac = float(kept.to(torch.float32).mean().item())
        assert _kept_fraction_ok(frac, got.numel(), keep), (n0, c, frac)
    lu.RECORD.append(dict(what="dropout_fwd %s N %d" % (geo, N), N=N, bytes=N * per * 2, worst_err=0.0, scale=0.0))


@pytest.mark.parametrize("geo", ["small", "large"])
def test_color_adjust_fwd_at_the_limit(geo):
    """rsu_color_adjust_fwd at keep 0.8 with the 16-channel output at the limit: three images on the host against the oracle (as
    tests/test_gpu_ops.py), every image's unmasked channels by their periodic source, the kept fraction of every chunk"""
    H, W = GEO[geo]
    keep, key = 0.8, 0xC0FFEE11
    N = lu.entry_n_max("rsu_color_adjust_fwd", H, W)
    rng = np.random.RandomState(H + 81)
    x = rng.rand(K, H, W, 3).astype(np.float32)
    x[np.abs(x - 0.5) < 1e-3] = 0.75   # (x - 0.5 never rounds to zero: a dropped element is then told from a kept one)
    w0, b0 = _rand(rng, 3, 3, scale=0.5), _rand(rng, 3, scale=0.1)
    xd, w0d, b0d = lu.periodic(x, N, torch.float32), hu.dev_f32(w0), hu.dev_f32(b0)
    out = lu.nan_out((N, H, W, 16))
    call("rsu_color_adjust_fwd", hu.ptr(xd), hu.ptr(w0d), hu.ptr(b0d), hu.ptr(out), N * H * W, keep, key, hu.stream())
    inv = np.float32(1) / np.float32(keep)
    net = U.conv1x1_fwd(x, w0, b0, sub=0.5)
    for n in (0, lu.straddler(H * W * 32), N - 1):
        m = lu.mask_range(n * H * W * 3, H * W * 3, keep, key).reshape(H, W, 3)
        got = hu.host(out[n])
        hu.assert_bf16_close(got[..., 0:3], net[n % K] * m * inv, "color_adjust net0 image %d" % n)
        for ci in range(3):
            for cj in range(3):
                assert np.array_equal(got[..., 4 + 3 * ci + cj], hu.q((x[n % K][..., ci] - 0.5) * m[..., cj])), (n, ci, cj)
        assert np.array_equal(got[..., 13:16], m) and not got[..., 3].any()
    xc = torch.from_numpy(hu.q(x - 0.5)).to(hu.DEV).to(torch.bfloat16)   # [K][H][W][3]
    for n0, c in lu._chunks(out):
        got = out[n0:n0 + c]
        src = xc.unsqueeze(0).expand((c // K, K) + tuple(xc.shape[1:])).reshape((c, H, W, 3)) if c % K == 0 else xc[:c]
        m = got[..., 13:16]
        assert bool(((m == 0) | (m == 1)).all().item()) and not bool(got[..., 3].any().item())
        for ci in range(3):
            want = src[..., ci:ci + 1] * m   # (x - 0.5)[ci] * m[cj]: exact, m is 0 or 1
            assert bool((got[..., 4 + 3 * ci:7 + 3 * ci] == want).all().item()), (n0, ci)
        frac = float(m.to(torch.float32).mean().item())
        assert _kept_fraction_ok(frac, m.numel(), keep), (n0, c, frac)
        assert not bool(torch.isnan(got[..., 0:3]).any().item())
    lu.RECORD.append(dict(what="color_adjust_fwd %s N %d" % (geo, N), N=N, bytes=N * H * W * 32, worst_err=0.0, scale=0.0))


# ------------------------------------------------------------------------------------------- head, bias gradient
@pytest.mark.parametrize("geo", ["small", "large"])
def test_head_at_the_limit(geo):
    """rsu_head_fwd_bwd and rsu_head_eval at C = 64 with act at the limit: prob and dact per image; loss, dw, db and the evaluation sums are
    sums over all pixels: the oracle's per-image float64 values times the images' multiplicities"""
    H, W = GEO[geo]
    C = 64
    N = lu.entry_n_max("rsu_head_fwd_bwd", H, W, C)
    npix = N * H * W
    rng = np.random.RandomState(H + 91)
    act = lu.base_images(H + 92, (H, W, C), relu=True)
    w, b = _rand(rng, C, 2, scale=0.3), _rand(rng, 2, scale=0.1)
    labels = (rng.rand(K, H, W) < 0.2).astype(np.int64)
    mult = np.array([(N - k + K - 1) // K for k in range(K)], np.float64)   # images n with n % K == k
    assert mult.sum() == N
    inv = 1.0 / npix
    rp, rdact = np.zeros((K, H, W), np.float32), np.zeros((K, H, W, C), np.float32)
    loss = 0.0
    rdw, rdb = np.zeros((C, 2), np.float64), np.zeros(2, np.float64)
    ce_k, I_k, P_k, Y_k = np.zeros(K), np.zeros(K), np.zeros(K), np.zeros(K)
    for k in range(K):
        a2, l1 = act[k].reshape(-1, C), labels[k].reshape(-1)
        p, mean_loss, dl = U.softmax_ce(U.conv1x1_fwd(a2, w, b), l1)   # dl = dlogits / (H W)
        dl = dl * np.float32(H * W * inv)
        dx, dw_k, db_k = U.conv1x1_bwd(a2, w, dl)
        rp[k], rdact[k] = p.reshape(H, W), U.relu_bwd(a2, dx).reshape(H, W, C)
        ce_k[k] = float(mean_loss) * H * W
        rdw += mult[k] * np.asarray(dw_k, np.float64)
        rdb += mult[k] * np.asarray(db_k, np.float64)
        p64, y = p.astype(np.float64), (l1 == 1).astype(np.float64)
        I_k[k], P_k[k], Y_k[k] = (p64 * y).sum(), p64.sum(), y.sum()
    loss = float((mult * ce_k).sum())
    ad, wd, bd = lu.periodic(act, N), hu.dev_f32(w), hu.dev_f32(b)
    lab = lu.periodic(labels, N, torch.int64)
    prob, dact = lu.nan_out((N, H, W), torch.float32), lu.nan_out((N, H, W, C))
    dw, db = lu.nan_out((C, 2), torch.float32), lu.nan_out((2,), torch.float32)
    loss_sum = torch.zeros(1, dtype=torch.float32, device=hu.DEV)
    ws = torch.zeros(lib().rsu_head_ws_floats(npix, C), dtype=torch.float32, device=hu.DEV)
    call("rsu_head_fwd_bwd", hu.ptr(ad), hu.ptr(wd), hu.ptr(bd), hu.ptr(lab), hu.ptr(prob), hu.ptr(loss_sum), hu.ptr(dact), hu.ptr(dw), hu.ptr(db),
         hu.ptr(ws), npix, C, inv, hu.stream())
    lu.assert_f32_periodic(prob, rp, "head prob %s N %d" % (geo, N), rtol=1e-4, atol_scale=1e-6)   # (tests/test_gpu_ops.py test_head's)
    lu.assert_bf16_periodic(dact, rdact, "head dact %s N %d" % (geo, N))
    lu.assert_periodic_bits(prob, "head prob")
    lu.assert_periodic_bits(dact, "head dact")
    got_loss = float(hu.host(loss_sum)[0])
    print("head %s: loss/npix %.8f oracle %.8f" % (geo, got_loss / npix, loss / npix))
    assert abs(got_loss / npix - loss / npix) < 2e-5 * max(1.0, abs(loss / npix))
    hu.assert_f32_close(hu.host(dw), rdw, "head dw %s" % geo)
    hu.assert_f32_close(hu.host(db), rdb, "head db %s" % geo)
    lu.note("head dw %s (loss/npix %.8f, oracle %.8f)" % (geo, got_loss / npix, loss / npix), N, npix * C * 2, hu.host(dw), rdw)
    del dact, ws
    # the evaluation head: accumulators from zero
    prob2 = lu.nan_out((N, H, W), torch.float32)
    sums = torch.zeros(5, dtype=torch.float32, device=hu.DEV)
    hist = torch.zeros((2, 256), dtype=torch.int64, device=hu.DEV)
    ews = torch.zeros(lib().rsu_head_eval_ws_floats(npix, C), dtype=torch.float32, device=hu.DEV)
    call("rsu_head_eval", hu.ptr(ad), hu.ptr(wd), hu.ptr(bd), hu.ptr(lab), None, None, hu.ptr(prob2), hu.ptr(sums), hu.ptr(hist), hu.ptr(ews),
         npix, C, hu.stream())
    lu.assert_f32_periodic(prob2, rp, "head_eval prob %s N %d" % (geo, N), rtol=1e-4, atol_scale=1e-6)
    assert torch.equal(prob2, prob), "the evaluation head writes the training head's prob bits"
    ref_sums = np.array([loss, float(npix), (mult * I_k).sum(), (mult * P_k).sum(), (mult * Y_k).sum()])
    hu.assert_f32_close(hu.host(sums), ref_sums, "head_eval sums %s" % geo)
    lu.note("head_eval sums %s" % geo, N, npix * C * 2, hu.host(sums), ref_sums)
    # the histogram is exact: bins of the (checked) f32 prob of the first K images, times the multiplicities
    pk, want = hu.host(prob[:K]), np.zeros((2, 256), np.int64)
    for k in range(K):
        bins = np.minimum(255, (pk[k].reshape(-1) * np.float32(256)).astype(np.int64))
        for l in (0, 1):
            want[l] += int(mult[k]) * np.bincount(bins[labels[k].reshape(-1) == l], minlength=256)
    assert np.array_equal(hist.cpu().numpy(), want) and want.sum() == npix


@pytest.mark.parametrize("geo", ["small", "large"])
def test_bias_grad_at_the_limit(geo):
    H, W = GEO[geo]
    C = 64
    N = lu.entry_n_max("rsu_bias_grad", H, W, C)
    npix = N * H * W
    dz = lu.base_images(H + 95, (H, W, C), scale=0.1)
    mult = np.array([(N - k + K - 1) // K for k in range(K)], np.float64)
    ref = (mult[:, None] * dz.reshape(K, -1, C).astype(np.float64).sum(1)).sum(0)
    dzd = lu.periodic(dz, N)
    db = lu.nan_out((C,), torch.float32)
    ws = torch.zeros(lib().rsu_bias_grad_ws_floats(npix, C), dtype=torch.float32, device=hu.DEV)
    call("rsu_bias_grad", hu.ptr(dzd), hu.ptr(db), hu.ptr(ws), npix, C, hu.stream())
    hu.assert_f32_close(hu.host(db), ref, "bias_grad %s N %d" % (geo, N))
    lu.RECORD.append(dict(what="bias_grad %s N %d" % (geo, N), N=N, bytes=npix * C * 2,
                          worst_err=float(np.abs(hu.host(db) - ref).max()), scale=float(np.abs(ref).max())))


# ------------------------------------------------------------------------------------------- the whole net at its largest batch
def test_net_at_the_largest_batch_its_own_rule_admits():
    """UNet (L = 2, root 64, 12-pixel patches: the oracle on K patches is cheap) at the largest per-GPU batch its own rule names -- read
    from the rule's message, not restated -- one forward and backward pass over a periodic batch of K patches. Loss, every patch's
    probabilities and every gradient tensor against the oracle on the K patches with the tolerances of tests/test_gpu_net.py (its own
    _check): the gradient of the mean over a periodic batch is the multiplicity-weighted mean of the K per-patch gradients. One patch
    more is refused before anything is allocated or launched."""
    import re
    from road_segmentation_unet_amd._lib import RsuError
    from road_segmentation_unet_amd.unet import UNet, input_size_needed
    from tests.test_gpu_net import _check, _rel_errs
    L, root, P, dilated = 2, 64, 12, False
    with pytest.raises(RsuError) as e:
        UNet(L, root, dilated, 1 << 30, P, training=True)
    B = int(re.search(r"largest per-GPU batch is (\d+)", str(e.value)).group(1))
    S = input_size_needed(P, L)
    assert B == lu.entry_n_max("rsu_conv_first_fwd", S, S, root) and B > 10000
    with pytest.raises(RsuError, match="largest per-GPU batch is %d" % B):
        UNet(L, root, dilated, B + 1, P, training=True)
    rng = np.random.RandomState(3)
    X = rng.rand(K, S, S, 3).astype(np.float32)
    labels = (rng.rand(K, P, P) < 0.2).astype(np.int64)
    params = U.init_params(L, root, dilated, seed=4, bias_scale=0.05)
    mult = np.array([(B - k + K - 1) // K for k in range(K)], np.float64)
    refs = {}
    for emu in (True, False):
        loss, prob, grads = 0.0, np.zeros((K, P, P), np.float32), None
        for k in range(K):
            l_k, p_k, g_k = U.loss_and_grads(params, X[k:k + 1], labels[k:k + 1], L, root, dilated, emulate_bf16=emu)
            loss += mult[k] / B * l_k
            prob[k] = p_k[0]
            grads = {n: (grads[n] if grads else 0.0) + mult[k] / B * g_k[n].astype(np.float64) for n in g_k}
        refs[emu] = (loss, prob, {n: g.astype(np.float32) for n, g in grads.items()})
    m = UNet(L, root, dilated, B, P, params=params, training=True)
    m.x.copy_(lu.periodic(X, B, torch.float32))
    m.labels.copy_(lu.periodic(labels, B, torch.int64))
    m.forward_device()
    m.backward_device(1.0 / (B * P * P))
    torch.cuda.synchronize()
    loss = float(m.loss_sum.item()) / (B * P * P)
    grads = {n: m.g[n].detach().cpu().numpy().copy() for n in m.names}
    for t in grads.values():
        assert np.isfinite(t).all()
    noise = _rel_errs(refs[True][2], refs[False][2])
    for emu, (ptol, ltol, gtol, factor) in ((True, (4e-3, 2e-3, 2e-2, 1.0)), (False, (3e-2, 1e-2, 1e-1, 1.5))):
        rloss, rprob, rgrads = refs[emu]
        rp = torch.from_numpy(rprob).to(hu.DEV)
        full = B // K * K
        d = float((m.prob[:full].view(full // K, K, P, P) - rp.unsqueeze(0)).abs().max().item())
        if B > full:
            d = max(d, float((m.prob[full:] - rp[:B - full]).abs().max().item()))
        assert d <= ptol, ("prob of every patch", emu, d)
        worst = _check(loss, hu.host(m.prob[:K]), grads, (rloss, rprob, rgrads), ptol, ltol, gtol, "B = %d, emulate_bf16 %s" % (B, emu), noise, factor)
        print("net at B = %d (emulate_bf16 %s): loss %.6f oracle %.6f, worst prob err %.2e, worst grad rel err %s %.2e" % (B, emu, loss, rloss, d, worst[0], worst[1]))
        lu.RECORD.append(dict(what="net L=2 root=64 P=12 B=%d emulate_bf16=%s: prob err %.2e, worst grad rel err %.2e (%s), loss %.6f vs %.6f"
                              % (B, emu, d, worst[1], worst[0], loss, rloss), N=B, bytes=B * (S - 2) * (S - 2) * root * 2, worst_err=d, scale=1.0))
    lu.assert_periodic_bits(m.prob, "net prob")
    del m
