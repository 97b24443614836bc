"""CPU: global-norm gradient clipping on the host side -- the --clip_grad_norm flag and its parser, the float32 mirror of the device's
state record (unet.clip_scale) against float64 numpy, and the new entry points in include/rsu.h, the ctypes table and the library."""
import os
import re

import numpy as np
import pytest

from road_segmentation_unet_amd import _lib
from road_segmentation_unet_amd.cli import parse_options
from road_segmentation_unet_amd.model import EXTRA_FLAG_DEFS, Options, parse_clip_grad_norm
from road_segmentation_unet_amd.unet import clip_scale

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32, f64 = np.float32, np.float64
SYMBOLS = {"rsu_grad_norm": 6, "rsu_grad_norm_ws_floats": 1, "rsu_clip_state_bytes": 0, "rsu_update_table_run_clip": 8,
           "rsu_update_table_run_adam_clip": 10}


# ------------------------------------------------------------------------------------------- the flag
@pytest.mark.parametrize("value,want", [(0, 0.0), (0.0, 0.0), ("0", 0.0), (1, 1.0), ("2.5", 2.5), (1e-3, 1e-3), (1e30, 1e30), (np.float32(0.5), 0.5)])
def test_parse_clip_grad_norm_accepts(value, want):
    got = parse_clip_grad_norm(value)
    assert isinstance(got, float) and got == want


@pytest.mark.parametrize("value", [float("nan"), float("inf"), -float("inf"), -1.0, -1e-30, "nan", "inf", "-2", "one", "", None, True, [1.0]])
def test_parse_clip_grad_norm_rejects(value):
    with pytest.raises(ValueError):
        parse_clip_grad_norm(value)


def test_options_and_command_line():
    assert Options().clip_grad_norm == 0.0          # off by default
    assert Options(clip_grad_norm=1.5).clip_grad_norm == 1.5
    assert Options(clip_grad_norm="3").clip_grad_norm == 3.0
    for bad in (-1.0, float("nan"), float("inf"), "x"):
        with pytest.raises(ValueError):
            Options(clip_grad_norm=bad)
    assert parse_options([]).clip_grad_norm == 0.0
    assert parse_options(["--clip_grad_norm=0.25"]).clip_grad_norm == 0.25
    with pytest.raises(ValueError):
        parse_options(["--clip_grad_norm=-1"])
    d = [d for d in EXTRA_FLAG_DEFS if d[0] == "clip_grad_norm"]
    assert len(d) == 1 and d[0][1:3] == (float, 0.0) and "0 = off" in d[0][3]


# ------------------------------------------------------------------------------------------- the mirror
def _ref(sumsq, c):
    """float64 numpy: the record's norm and scale from the float32 sum of squares"""
    s = f64(f32(sumsq))
    norm = f32(np.sqrt(s))
    if f64(norm) > f64(f32(c)):
        return norm, f32(f64(f32(c)) / f64(norm))
    return norm, f32(1.0)


@pytest.mark.parametrize("sumsq,c", [(4.0, 3.0), (0.0, 1.0), (1e-12, 1e-3), (2.0, 1.5), (123456.0, 1e30),   # norm < c
                                     (9.0, 2.0), (2.0, 1.0), (1e10, 1.0), (3.0e38, 0.1), (1e-30, 1e-20), (16777215.0, 4000.0)])   # norm > c
def test_clip_scale_against_float64(sumsq, c):
    norm, scale = clip_scale(f32(sumsq), c)
    assert isinstance(norm, f32) and isinstance(scale, f32)
    rn, rs = _ref(sumsq, c)
    assert norm == rn and scale == rs
    if f64(rn) > f64(f32(c)):
        assert scale < 1 and abs(f64(scale) * f64(norm) / f64(f32(c)) - 1.0) <= 2.0 ** -23   # the clipped gradient has norm c
    else:
        assert scale == 1


def test_clip_scale_is_exactly_one_at_the_bound():
    for sumsq in (4.0, 2.0, 1e-6, 12345.0):
        norm, _ = clip_scale(f32(sumsq), 1e30)
        assert clip_scale(f32(sumsq), float(norm)) == (norm, f32(1.0))                       # norm == c: not clipped
        below = np.nextafter(norm, f32(0))
        n2, s2 = clip_scale(f32(sumsq), float(below))
        assert n2 == norm and s2 < 1 and s2 == f32(f64(below) / f64(norm))                   # one ulp below: clipped


@pytest.mark.parametrize("sumsq", [float("inf"), float("nan")])
def test_clip_scale_of_a_sum_that_is_not_finite_is_zero(sumsq):
    norm, scale = clip_scale(f32(sumsq), 1.0)
    assert scale == 0 and isinstance(scale, f32) and not np.isfinite(norm)
    with np.errstate(over="ignore"):
        assert clip_scale(f32(3.0e38) * f32(2), 1e30)[1] == 0   # the float32 overflow of the sum


# ------------------------------------------------------------------------------------------- the ABI
def test_symbols_are_declared_and_exported():
    txt = open(os.path.join(ROOT, "include", "rsu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = _lib.lib()
    for name, nargs in SYMBOLS.items():
        m = re.search(r"\b%s\s*\(([^)]*)\)" % name, code)
        assert m, "%s is not declared in rsu.h" % name
        args = [a for a in m.group(1).split(",") if a.strip() not in ("", "void")]
        assert len(args) == nargs == len(_lib.SIGNATURES[name][1]), name
        assert hasattr(L, name), "librsu_hip.so does not export %s" % name
    assert "float* ws, void* state, rsu_stream_t stream" in code and code.count("const void* state, rsu_stream_t stream") == 2


def test_record_constants_agree():
    txt = open(os.path.join(ROOT, "include", "rsu.h")).read()
    defs = dict(re.findall(r"#define (RSU_CLIP_[A-Z_]+|RSU_GRAD_NORM_BLOCK_FLOATS) (\d+)", txt))
    assert int(defs["RSU_CLIP_STATE_BYTES"]) == _lib.CLIP_STATE_BYTES == 32 == _lib.lib().rsu_clip_state_bytes()
    assert (int(defs["RSU_CLIP_CLIPPED"]), int(defs["RSU_CLIP_NONFINITE"])) == (_lib.CLIP_CLIPPED, _lib.CLIP_NONFINITE) == (1, 2)
    share = int(defs["RSU_GRAD_NORM_BLOCK_FLOATS"])
    assert share == _lib.GRAD_NORM_BLOCK_FLOATS and share % (4 * 256) == 0
    ws = _lib.lib().rsu_grad_norm_ws_floats
    # two floats per workgroup, a grid that n alone fixes; n < 1 has no workspace
    assert [ws(n) for n in (-1, 0, 1, 3, 4, share, share + 3, share + 4, 2 * share, 2 * share + 4)] == [0, 0, 2, 2, 2, 2, 2, 4, 4, 6]


def test_pure_host_argument_checks():
    """what rsu_grad_norm and the _clip runs reject before anything is launched (no device is touched)"""
    L = _lib.lib()
    a = 0x1000   # an aligned address that is never dereferenced: every call below fails its checks
    assert L.rsu_grad_norm(None, 8, 1.0, a, a, None) == -22
    assert L.rsu_grad_norm(a, 0, 1.0, a, a, None) == -22
    assert L.rsu_grad_norm(a, -4, 1.0, a, a, None) == -22
    assert L.rsu_grad_norm(a + 4, 8, 1.0, a, a, None) == -22          # g must be 16-byte aligned
    assert L.rsu_grad_norm(a, 8, 1.0, None, a, None) == -22
    assert L.rsu_grad_norm(a, 8, 1.0, a, None, None) == -22
    for bad in (0.0, -1.0, float("nan")):
        assert L.rsu_grad_norm(a, 8, bad, a, a, None) == -22
    assert L.rsu_update_table_run_clip(a, 1, 1, 0.01, 0.9, 1.0, None, None) == -22
    assert L.rsu_update_table_run_adam_clip(a, 1, 1, 1e-3, 0.9, 0.999, 1e-8, 1.0, None, None) == -22
    assert L.rsu_update_table_run_clip(None, 1, 1, 0.01, 0.9, 1.0, a, None) == -22
    assert L.rsu_update_table_run_adam_clip(a, 0, 1, 1e-3, 0.9, 0.999, 1e-8, 1.0, a, None) == -22
