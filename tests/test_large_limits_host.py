"""The 2-GiB tensor limit of every batch-taking entry point, on the host (no GPU is needed: the addresses are never dereferenced, each
call fails its size check before anything is launched). tests/large_util.LIMITS states each entry's limit as bytes per image; here the
C ABI returns RSU_E2BIG and _lib.call raises its 2-GiB RsuError at n_max + 1 of that table, for a geometry with many small images and one
with few large ones, so the C and the Python statements of the limit cannot drift apart; tests/test_gpu_large_tensors.py runs the same
entries at n_max of the same table, where they must succeed. UNet's own largest-batch rule is held to the same limit."""
import ctypes

import numpy as np
import pytest

from oracle import unet_oracle as U
from road_segmentation_unet_amd import _lib
from road_segmentation_unet_amd._lib import RsuError, RsuSrc, RsuWgradJob
from tests import large_util as lu

P = 4096   # (a device address that is never dereferenced: every call below is refused)
p = ctypes.c_void_p(P)
SMALL, LARGE = (66, 66), (260, 258)


def _src(H, W, C):
    return RsuSrc(P, H, W, C, 0, 0)


def _conv_fwd(N, H, W, Cin, Cout, dil=1):
    return ((RsuSrc * 1)(_src(H, W, Cin)), 1, p, p, p, N, H, W, Cout, dil, 1, 0, None)


def _conv_fwd_pool(N, H, W, Cin, Cout):
    return ((RsuSrc * 1)(_src(H, W, Cin)), 1, p, p, p, p, p, N, H, W, Cout, 1.0, 0, 0, None)


def _conv_bwd_data(N, H, W, Cin, Cout, dil=1):
    return (p, p, p, p, 0, N, H, W, Cin, 0, Cin, Cout, dil, 0, None)


def _conv_bwd_weight(N, H, W, Cin, Cout, dil=1):
    return (ctypes.byref(_src(H, W, Cin)), p, p, p, p, N, H - 2 * dil, W - 2 * dil, Cin, 0, Cout, dil, 0, None)


_KEEP = []


def _group_plan(N, H, W, Cin, Cout, dil=1):
    jobs = (RsuWgradJob * 1)(RsuWgradJob(_lib.WGRAD_CONV3X3, _src(H, W, Cin), P, P, P, H - 2 * dil, W - 2 * dil, Cin, 0, Cout, dil))
    table = ctypes.create_string_buffer(_lib.lib().rsu_wgrad_group_table_bytes())
    _KEEP[:] = [jobs, table]
    return (jobs, 1, p, N, 0, table)


def _convT(N, H, W, Cin, Cout):
    return (p, p, p, p, N, H, W, Cin, Cout, 0, None)


# entry -> (argument builder, geometry without the image size). Geometries: the shapes tests/test_gpu_large_tensors.py runs at n_max.
ENTRIES = {
    "rsu_conv2d_fwd": (_conv_fwd, (64, 64)),
    "rsu_conv2d_fwd_pool": (_conv_fwd_pool, (64, 64)),
    "rsu_conv2d_bwd_data": (_conv_bwd_data, (64, 64)),
    "rsu_conv2d_bwd_weight": (_conv_bwd_weight, (64, 64)),
    "rsu_wgrad_group_plan": (_group_plan, (64, 64)),
    "rsu_convT2x2_fwd": (_convT, (64, 32)),
    "rsu_convT2x2_bwd_data": (lambda N, H, W, Cin, Cout: (p, p, p, p, 1.0, N, H, W, Cin, Cout, 0, None), (64, 32)),
    "rsu_convT2x2_bwd_weight": (lambda N, H, W, Cin, Cout: (p, p, p, p, p, N, H, W, Cin, Cout, 0, None), (64, 32)),
    "rsu_conv_first_fwd": (lambda N, H, W, Cout: (p, p, p, p, N, H, W, Cout, 1, 0, None), (64,)),
    "rsu_color_conv_first_fwd": (lambda N, H, W, Cout: (p, p, p, p, p, p, N, H, W, Cout, 1, 0, None), (64,)),
    "rsu_conv_first_bwd_weight": (lambda N, H, W, Cout: (p, p, p, p, p, p, N, H, W, Cout, 1, 0, None), (64,)),
    "rsu_maxpool2x2_fwd_code": (lambda N, H, W, C: (p, p, p, N, H, W, C, 0.8, 7, None), (64,)),
    "rsu_pool_skip_relu_bwd_code": (lambda N, H, W, C: (None, p, p, p, p, N, H, W, C, H - 8, W - 8, 0.8, 7, None), (64,)),
    "rsu_pool_skip_relu_bwd": (lambda N, H, W, C: (p, p, p, p, N, H, W, C, H - 8, W - 8, 0.8, 7, None), (64,)),
    "rsu_dropout_fwd": (lambda N, H, W, C: (p, p, N * H * W * C, 0.8, 7, None), (64,)),
    "rsu_color_adjust_fwd": (lambda N, H, W: (p, p, p, p, N * H * W, 0.8, 7, None), ()),
    "rsu_head_fwd_bwd": (lambda N, H, W, C: (p, p, p, p, p, p, p, p, p, p, N * H * W, C, 1e-6, None), (64,)),
    "rsu_head_eval": (lambda N, H, W, C: (p, p, p, p, None, None, p, p, p, p, N * H * W, C, None), (64,)),
    "rsu_bias_grad": (lambda N, H, W, C: (p, p, p, N * H * W, C, None), (64,)),
}


def test_the_table_covers_every_entry():
    assert sorted(ENTRIES) == sorted(lu.LIMITS)
    assert lu.n_max(1) == lu.LIMIT - 1 and lu.n_max(lu.LIMIT) == 0 and lu.n_max(16) * 16 < lu.LIMIT <= (lu.n_max(16) + 1) * 16


@pytest.mark.parametrize("H,W", [SMALL, LARGE])
@pytest.mark.parametrize("name", sorted(ENTRIES))
def test_entry_refuses_one_image_more_than_its_limit(name, H, W):
    """N = n_max + 1 of the table: RSU_E2BIG from the C ABI, the 2-GiB RsuError from _lib.call; and the table's n_max is the last batch
    whose largest tensor stays below the limit (the GPU tests run that batch)"""
    build, geo = ENTRIES[name]
    per = max(lu.LIMITS[name](H, W, *geo))
    N = lu.entry_n_max(name, H, W, *geo)
    assert N * per < lu.LIMIT <= (N + 1) * per and N >= 100
    fn = getattr(_lib.lib(), name)
    assert fn(*build(N + 1, H, W, *geo)) == _lib.E2BIG, name
    with pytest.raises(RsuError, match="reaches 2 GiB"):
        _lib.call(name, *build(N + 1, H, W, *geo))


def test_conv_limit_applies_to_input_and_output_and_every_source():
    """32 -> 64 channels: the OUTPUT reaches the limit first; 64 -> 32 and dilation 2: the input; a second, larger concat source"""
    L = _lib.lib()
    H, W = SMALL
    n_out = lu.n_max((H - 2) * (W - 2) * 64 * 2)
    assert n_out * H * W * 32 * 2 < lu.LIMIT
    assert L.rsu_conv2d_fwd(*_conv_fwd(n_out + 1, H, W, 32, 64)) == _lib.E2BIG
    n_in = lu.n_max(H * W * 64 * 2)
    assert L.rsu_conv2d_fwd(*_conv_fwd(n_in + 1, H, W, 64, 32, 2)) == _lib.E2BIG
    big = lu.n_max(90 * 90 * 32 * 2)   # a skip tensor of 90 x 90 cropped to the 66 x 66 window
    srcs = (RsuSrc * 2)(RsuSrc(P, 90, 90, 32, 12, 12), _src(H, W, 32))
    assert L.rsu_conv2d_fwd(srcs, 2, p, p, p, big + 1, H, W, 32, 1, 1, 0, None) == _lib.E2BIG
    s = RsuSrc(P, 90, 90, 32, 12, 12)
    assert L.rsu_conv2d_bwd_weight(ctypes.byref(s), p, p, p, p, big + 1, H - 2, W - 2, 64, 0, 32, 1, 0, None) == _lib.E2BIG


def test_heads_and_pools_refuse_at_the_limit_in_every_form():
    """the entries that had no size check before: all heads, both pools, with and without dropout (the 32-bit dropout counter and the
    int products of the junction kernel stay in range because the tensor does)"""
    L = _lib.lib()
    H, W = SMALL
    N = lu.n_max(H * W * 64 * 2) + 1
    npix = N * H * W
    assert L.rsu_head_fwd(p, p, p, p, p, npix, 64, None) == _lib.E2BIG
    assert L.rsu_head_fwd_bwd_w(p, p, p, p, None, None, p, p, p, p, p, p, p, npix, 64, 1e-6, None) == _lib.E2BIG
    assert L.rsu_head_dice_sums(p, p, p, p, None, p, p, p, npix, 64, None) == _lib.E2BIG
    assert L.rsu_head_fwd_bwd_dice(p, p, p, p, None, None, p, 1.0, 1.0, p, p, p, p, p, p, p, npix, 64, 1e-6, None) == _lib.E2BIG
    assert L.rsu_head_fwd_bwd_focal(p, p, p, p, None, None, 2.0, None, 0.0, 0.0, p, p, p, p, p, p, p, npix, 64, 1e-6, None) == _lib.E2BIG
    assert L.rsu_head_eval_focal(p, p, p, p, None, None, 2.0, p, p, p, p, npix, 64, None) == _lib.E2BIG
    assert L.rsu_head_fwd(p, p, p, p, p, lu.n_max(16) + 1, 8, None) == _lib.E2BIG   # C = 8: 16 bytes per pixel
    for keep in (1.0, 0.8):
        assert L.rsu_maxpool2x2_fwd(p, p, N, H, W, 64, keep, 7, None) == _lib.E2BIG
        assert L.rsu_maxpool2x2_fwd_code(p, p, None, N, H + 1, W, 64, keep, 7, None) == _lib.E2BIG   # odd H, no code bytes
        assert L.rsu_pool_skip_relu_bwd(p, None, None, p, N, H + 1, W, 64, 0, 0, keep, 7, None) == _lib.E2BIG
        assert L.rsu_dropout_fwd(p, p, N * H * W * 64, keep, 7, None) == _lib.E2BIG
        assert L.rsu_color_adjust_fwd(p, p, p, p, lu.n_max(32) + 1, keep, 7, None) == _lib.E2BIG
    # what was RSU_EINVAL before stays refused; a bad argument is still RSU_EINVAL whatever the size
    assert L.rsu_dropout_fwd(p, p, 1 << 33, 0.8, 7, None) == _lib.E2BIG
    assert L.rsu_dropout_fwd(p, p, (1 << 33) + 4, 0.8, 7, None) == -22
    assert L.rsu_dropout_fwd(p, p, N * H * W * 64, 1.5, 7, None) == -22
    assert L.rsu_head_fwd(p, p, p, p, p, npix, 24, None) == -22
    assert L.rsu_bias_grad(p, p, None, npix, 64, None) == -22


def test_transposed_conv_paths_above_the_limit_are_refusals_not_fallbacks():
    """rsu_convT2x2_fwd / _bwd_data leave igemm_ct for the generic launch when the 4x tensor reaches the limit, and igemm_wgt / igemm_wg1
    decline at 2^28 pixels -- but the generic launches they fall to refuse the same tensors: with 8 channels (the fewest) 2^28 input
    pixels are 4 GiB of bf16, so the pixel-count branches cannot be reached below the byte limit, and every such call is RSU_E2BIG"""
    L = _lib.lib()
    assert (1 << 28) * 8 * 2 > lu.LIMIT
    H, W = LARGE
    for cin, cout in ((64, 32), (8, 8), (32, 64)):
        N = lu.n_max(max(lu.LIMITS["rsu_convT2x2_fwd"](H, W, cin, cout))) + 1
        assert L.rsu_convT2x2_fwd(*_convT(N, H, W, cin, cout)) == _lib.E2BIG
        assert L.rsu_convT2x2_bwd_data(p, p, p, None, 1.0, N, H, W, cin, cout, 0, None) == _lib.E2BIG
        assert L.rsu_convT2x2_bwd_weight(p, p, p, p, p, N, H, W, cin, cout, 0, None) == _lib.E2BIG
    n28 = (1 << 28) // (H * W) + 1
    assert L.rsu_convT2x2_bwd_weight(p, p, p, p, p, n28, H, W, 8, 8, 0, None) == _lib.E2BIG
    assert L.rsu_conv_first_bwd_weight(p, p, p, p, p, p, n28, H, W, 8, 1, 0, None) == _lib.E2BIG


def test_unet_batch_rule_is_the_abi_limit():
    """UNet._check_tensor_sizes names the largest batch from the level-0 tensors (the 16-channel input tensor and the first conv's
    output): the batch it names is n_max of the first-conv entry of the table, the one the C ABI still takes, and one more is refused by
    both -- by UNet before anything is allocated or launched (no device is needed to see it)"""
    from road_segmentation_unet_amd.unet import UNet, input_size_needed
    for L_, root, P_ in ((2, 64, 20), (2, 64, 200), (5, 64, 388)):
        S = input_size_needed(P_, L_)
        nmax = lu.entry_n_max("rsu_conv_first_fwd", S, S, root)
        with pytest.raises(RsuError, match="largest per-GPU batch is %d$" % nmax):
            UNet(L_, root, False, nmax + 1, P_, device="cpu", params=None, training=True)
        assert _lib.lib().rsu_conv_first_fwd(p, p, p, p, nmax + 1, S, S, root, 1, 0, None) == _lib.E2BIG


def test_mask_range_is_the_oracles_dropout_mask():
    for keep, key in ((0.8, 0x1234ABCD), (0.5, 7)):
        full = U.dropout_mask((5000,), keep, key)
        assert np.array_equal(lu.mask_range(0, 5000, keep, key), full)
        assert np.array_equal(lu.mask_range(1234, 3000, keep, key), full[1234:4234])
    m = lu.mask_range((1 << 30) - 50, 100, 0.8, 3)   # across 2^30: plain counters, no wrap
    assert m.shape == (100,) and set(np.unique(m)) <= {0.0, 1.0}


def test_the_chunked_comparison_sees_one_wrong_element_and_names_it(monkeypatch):
    """tests/large_util's device-side comparison, run here on the CPU with small chunks: a periodic batch passes, one element off by two
    bf16 ulps, one NaN left behind and one foreign image each fail, and the message names the image and the byte offset"""
    import torch
    from tests import hiputil as hu
    monkeypatch.setattr(hu, "DEV", "cpu")
    monkeypatch.setattr(lu, "CHUNK_BYTES", 7 * 5 * 6 * 8 * 2 + 3)   # a chunk of 6 images (whole periods), N = 20: 3 chunks + a tail of 2
    base = lu.base_images(3, (5, 6, 8))
    assert base.shape == (lu.K, 5, 6, 8)
    N = 20
    x = lu.periodic(base, N)
    assert [c for _, c in lu._chunks(x)] == [6, 6, 6, 2]
    for n in range(N):
        assert np.array_equal(x[n].float().numpy(), base[n % lu.K])
    ref = base.astype(np.float64) * (1 + 2.0 ** -10)   # inside one ulp
    lu.assert_bf16_periodic(x, ref.astype(np.float32), "clean")
    lu.assert_periodic_bits(x, "clean")
    lu.assert_f32_periodic(x.float(), base, "clean f32")
    per = 5 * 6 * 8
    for n, e, v in ((19, 7, None), (13, per - 1, float("nan")), (0, 0, None)):
        y = x.clone()
        flat = y.view(N, per)
        big = int(np.argmax(np.abs(base[n % lu.K].reshape(-1)))) if v is None else e
        flat[n, big] = flat[n, big] * (1 + 2.0 ** -6) if v is None else v
        with pytest.raises(AssertionError, match=r"worst in image %d of 20 at byte offset %d " % (n, (n * per + big) * 2)):
            lu.assert_bf16_periodic(y, base, "planted")
        if v is None:
            with pytest.raises(AssertionError, match="image %d differs" % n if n >= lu.K else "differs"):
                lu.assert_periodic_bits(y, "planted")
    y = x.clone()
    y[17] = x[16]   # a foreign image: what a wrapped offset reads
    with pytest.raises(AssertionError, match="image 17 of 20"):
        lu.assert_bf16_periodic(y, base, "foreign")
    z = lu.sparse({4: base[1]}, 9, (5, 6, 8))
    assert not z[3].any() and not z[5].any() and np.array_equal(z[4].float().numpy(), base[1])
