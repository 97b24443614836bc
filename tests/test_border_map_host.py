"""The host side of the border-distance weight map that needs no GPU: hostio.border_weight_map (the CPU statement of include/rsu.h
rsu_border_map) against the brute-force definition, its D4 equivariance, the --border_weight / --border_sigma options and the command
line, and the ABI's argument checks (host code)."""
import ctypes
import glob
import os

import numpy as np
import pytest
import torch

from road_segmentation_unet_amd import hostio
from road_segmentation_unet_amd.cli import parse_options
from road_segmentation_unet_amd.model import EXTRA_FLAG_DEFS, FLAG_DEFS, Options
from road_segmentation_unet_amd.pool import d4_apply
from tests import border_util as bu

SIZES = [(20, 20), (37, 41), (41, 37)]
CASES = sorted(bu.case_tiles(4, 4))


@pytest.mark.parametrize("with_mul", [False, True])
@pytest.mark.parametrize("H,W", SIZES)
def test_host_map_equals_the_brute_force_definition(H, W, with_mul):
    tiles = bu.case_tiles(H, W)
    labels = np.stack([tiles[k] for k in CASES])
    rng = np.random.RandomState(H + W)
    for w0, sigma in ((10.0, 5.0), (3.5, 1.25), (0.0, 5.0)):
        mul = bu.mul_map(rng, labels) if with_mul else None
        out, d2 = hostio.border_weight_map(labels, w0, sigma, mul=mul)
        ref, rd2 = bu.brute_map(labels, w0, sigma, mul=mul)
        assert out.dtype == np.float32 and d2.dtype == np.int32 and out.shape == d2.shape == labels.shape
        assert np.array_equal(d2, rd2)                                     # exact
        err = float(np.abs(out.astype(np.float64) - ref).max())
        print("H %d W %d w0 %g sigma %g mul %s: max |out - float64| %.3e (bound %.3e)" % (H, W, w0, sigma, with_mul, err, bu.tolerance(w0, mul)))
        assert err <= bu.tolerance(w0, mul)
        ign = (labels != 0) & (labels != 1)
        assert ign.any() and not np.any(out[ign]) and not np.any(np.signbit(out[ign])) and np.all(d2[ign] == bu.D2_INF)   # +0, never NaN
        for k in ("all0", "all1", "only_ignored_other"):                   # no other class in the tile: all ones, D2_INF
            i = CASES.index(k)
            v = ~ign[i]
            assert np.all(d2[i] == bu.D2_INF)
            assert np.array_equal(out[i][v], np.ones(v.sum(), np.float32) if mul is None else mul[i][v])
        assert d2[(labels == 0) | (labels == 1)].min() == 1                # border pixels


def test_border_pixels_have_d2_one_and_a_2d_input_works():
    t = np.zeros((5, 6), dtype=np.int64)
    t[2, 3] = 1
    out, d2 = hostio.border_weight_map(t, 10.0, 5.0)
    assert out.shape == d2.shape == (5, 6)
    assert d2[2, 3] == 1 and d2[2, 2] == 1 and d2[1, 3] == 1 and d2[1, 2] == 2 and d2[0, 0] == 13 and d2[4, 5] == 8
    assert out[2, 3] == np.float32(1.0 + 10.0 * np.exp(-1.0 / 50.0)) or abs(float(out[2, 3]) - (1.0 + 10.0 * np.exp(-1.0 / 50.0))) <= bu.tolerance(10.0)
    for bad in (dict(w0=-1.0, sigma=5.0), dict(w0=float("nan"), sigma=5.0), dict(w0=1.0, sigma=0.0), dict(w0=1.0, sigma=float("inf"))):
        with pytest.raises(ValueError):
            hostio.border_weight_map(t, **bad)
    with pytest.raises(ValueError):
        hostio.border_weight_map(t.astype(np.float32), 1.0, 5.0)


def test_d4_equivariance_is_exact():
    """the map of d4_apply(labels, op) is d4_apply(map, op), bit for bit, for all 16 ops: the definition has no preferred axis"""
    tiles = bu.case_tiles(24, 24, seed=3)
    for name in ("iid_ignored", "diagonal", "straight_ignored"):
        lab = tiles[name]
        out, d2 = hostio.border_weight_map(lab, 10.0, 5.0)
        for ud in (False, True):
            for lr in (False, True):
                for tr in (False, True):
                    for k in (0, 1, 2, 3):
                        op = (ud, lr, tr, k)
                        lab_t = d4_apply(torch.from_numpy(lab), op).contiguous().numpy()
                        out_t, d2_t = hostio.border_weight_map(lab_t, 10.0, 5.0)
                        assert np.array_equal(d2_t, d4_apply(torch.from_numpy(d2), op).numpy()), (name, op)
                        assert np.array_equal(out_t.view(np.int32), d4_apply(torch.from_numpy(out), op).contiguous().numpy().view(np.int32)), (name, op)


def test_border_options_and_command_line():
    assert len(FLAG_DEFS) == 30                                            # the reference's flags stay the reference's
    defs = {d[0]: d for d in EXTRA_FLAG_DEFS}
    assert defs["border_weight"][1:3] == (float, 0.0) and defs["border_sigma"][1:3] == (float, 5.0)
    assert "mean weight" in defs["border_weight"][3] and "step size" in defs["border_weight"][3]
    o = Options()
    assert o.border_weight == 0.0 and o.border_sigma == 5.0
    o = Options(border_weight="10", border_sigma=2)
    assert o.border_weight == 10.0 and o.border_sigma == 2.0 and isinstance(o.border_sigma, float)
    assert Options(border_weight=0).border_weight == 0.0
    for bad in (-1.0, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError):
            Options(border_weight=bad)
    for bad in (0.0, -2.0, float("nan"), float("inf"), "x", None):
        with pytest.raises(ValueError):
            Options(border_sigma=bad)
    o = parse_options([])
    assert o.border_weight == 0.0 and o.border_sigma == 5.0
    o = parse_options(["--border_weight=10", "--border_sigma", "3.5", "--d4_augmentation"])
    assert o.border_weight == 10.0 and o.border_sigma == 3.5 and o.d4_augmentation is True
    with pytest.raises(ValueError):
        parse_options(["--border_weight=-1"])
    with pytest.raises(ValueError):
        parse_options(["--border_sigma=0"])


def test_abi_refuses_bad_arguments_on_the_host():
    """every refused value returns RSU_EINVAL (or RSU_E2BIG) from host code, before anything is launched (no GPU is needed to see it; the
    pointers are never dereferenced); the workspace size is one word per pixel, 0 for a refused size"""
    from road_segmentation_unet_amd import _lib
    L = _lib.lib()
    assert _lib.BORDER_D2_INF == bu.D2_INF == hostio.BORDER_D2_INF == 2 ** 31 - 1
    assert L.rsu_border_map_ws_bytes(4, 388, 388) == 4 * 388 * 388 * 4
    assert L.rsu_border_map_ws_bytes(1, _lib.BORDER_MAX_SIDE, _lib.BORDER_MAX_SIDE) > 0
    for n, h, w in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-1, 8, 8), (1, _lib.BORDER_MAX_SIDE + 1, 8), (1, 8, _lib.BORDER_MAX_SIDE + 1)):
        assert L.rsu_border_map_ws_bytes(n, h, w) == 0
    p = ctypes.c_void_p(4096)   # (never dereferenced: every call below is refused)
    ok = dict(labels=p, mul=None, out=p, d2=None, ws=p, N=1, H=8, W=8, w0=10.0, sigma=5.0)
    nan, inf = float("nan"), float("inf")
    bad = [dict(labels=None), dict(out=None), dict(ws=None), dict(N=0), dict(H=0), dict(W=0), dict(N=-3), dict(H=_lib.BORDER_MAX_SIDE + 1),
           dict(W=_lib.BORDER_MAX_SIDE + 1), dict(w0=-1.0), dict(w0=nan), dict(w0=inf), dict(sigma=0.0), dict(sigma=-1.0), dict(sigma=nan),
           dict(sigma=inf)]
    for b in bad:
        a = dict(ok, **b)
        rc = L.rsu_border_map(a["labels"], a["mul"], a["out"], a["d2"], a["ws"], a["N"], a["H"], a["W"], a["w0"], a["sigma"], None)
        assert rc == -22, (b, rc)
    assert L.rsu_border_map(p, None, p, None, p, 300, 1024, 1024, 10.0, 5.0, None) == _lib.E2BIG   # 2.5 GB of labels


def test_kernel_isa_has_no_fused_multiply_add():
    """hostio.border_weight_map restates the kernel's float32 arithmetic operation by operation: the compiled kernel must round every
    multiply and add on its own (csrc/Makefile compiles border_map.hip with -ffp-contract=off). Reads the ISA the build keeps."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    isa = glob.glob(os.path.join(root, "road_segmentation_unet_amd", "csrc", "build", "border_map-hip-*gfx950.s"))
    assert isa, "build() keeps the ISA of every kernel file (-save-temps=obj)"
    text = open(isa[0]).read()
    for fused in ("v_fma_f32", "v_fmac_f32", "v_fmaak_f32", "v_fmamk_f32", "v_mad_f32", "v_mac_f32", "v_pk_fma_f32"):
        assert fused not in text, fused
    assert "v_mul_f32" in text and "v_rndne_f32" in text
