"""The host side of the soft-Dice loss term that needs no GPU: the --dice_weight / --dice_smooth options, dice_from_sums, and the new
entry points in the ctypes table and the header."""
import os
import re

import numpy as np
import pytest

from road_segmentation_unet_amd import _lib
from road_segmentation_unet_amd import model as M
from road_segmentation_unet_amd.cli import parse_options

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("rsu_head_dice_ws_floats", "rsu_head_dice_sums", "rsu_head_fwd_bwd_dice")


def test_dice_options_defaults_and_values():
    o = M.Options()
    assert o.dice_weight == 0.0 and o.dice_smooth == 1.0
    o = M.Options(dice_weight="0.7", dice_smooth=2)
    assert o.dice_weight == 0.7 and o.dice_smooth == 2.0 and isinstance(o.dice_smooth, float)
    assert M.parse_dice_weight(0) == 0.0 and M.parse_dice_weight(" 1e-1 ") == 0.1
    assert M.parse_dice_smooth("1e-6") == 1e-6


@pytest.mark.parametrize("bad", [-0.5, "-1", float("nan"), "nan", float("inf"), "x", None, (1.0, 2.0)])
def test_dice_weight_rejects(bad):
    with pytest.raises(ValueError):
        M.parse_dice_weight(bad)
    with pytest.raises(ValueError):
        M.Options(dice_weight=bad)


@pytest.mark.parametrize("bad", [0.0, "0", -1.0, float("nan"), float("inf"), "-inf", "s", None])
def test_dice_smooth_rejects(bad):
    with pytest.raises(ValueError):
        M.parse_dice_smooth(bad)
    with pytest.raises(ValueError):
        M.Options(dice_smooth=bad)


def test_command_line_flags_are_project_flags():
    extra = {d[0]: d for d in M.EXTRA_FLAG_DEFS}
    assert extra["dice_weight"][1:3] == (float, 0.0) and extra["dice_smooth"][1:3] == (float, 1.0)
    assert len(M.FLAG_DEFS) == 30 and not any(d[0].startswith("dice") for d in M.FLAG_DEFS)   # the reference's 30 flags stay its own
    o = parse_options([])
    assert o.dice_weight == 0.0 and o.dice_smooth == 1.0
    o = parse_options(["--dice_weight=0.7", "--dice_smooth", "0.5"])
    assert o.dice_weight == 0.7 and o.dice_smooth == 0.5
    for argv in (["--dice_weight=-1"], ["--dice_weight=nan"], ["--dice_smooth=0"], ["--dice_smooth=inf"]):
        with pytest.raises(ValueError):
            parse_options(argv)


def test_dice_from_sums_against_a_direct_dice():
    rng = np.random.RandomState(0)
    n = 5000
    p = rng.rand(n)
    y = (rng.rand(n) < 0.2).astype(np.float64)
    m = np.where(rng.rand(n) < 0.1, 0.0, 0.25 + rng.rand(n))
    for s in (1.0, 1e-3, 17.0):
        direct = (2.0 * np.sum(m * p * y) + s) / (np.sum(m * p) + np.sum(m * y) + s)
        got = M.dice_from_sums(np.sum(m * p * y), np.sum(m * p), np.sum(m * y), s)
        assert got == pytest.approx(direct, rel=1e-15)
        assert 0.0 < got < 1.0
    # a perfect prediction of a hard mask: D = 1; nothing counted at all: D = 1 (1 - D = 0: no loss from an empty batch)
    assert M.dice_from_sums(y.sum(), y.sum(), y.sum(), 1.0) == 1.0
    assert M.dice_from_sums(0.0, 0.0, 0.0, 1.0) == 1.0
    assert M.dice_from_sums(0.0, 0.0, 0.0, 1e-6) == 1.0
    # arrays pass through element-wise (the model applies it to device tensors)
    out = M.dice_from_sums(np.array([0.0, 1.0]), np.array([0.0, 2.0]), np.array([0.0, 3.0]), 1.0)
    assert out.tolist() == [1.0, 0.5]


def test_new_entry_points_in_the_ctypes_table_and_the_header():
    header = open(os.path.join(ROOT, "include", "rsu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for s in NEW_SYMBOLS:
        assert s in _lib.SIGNATURES, s
        assert re.search(r"\b%s\s*\(" % s, code), "include/rsu.h does not declare %s" % s
    assert _lib.SIGNATURES["rsu_head_dice_ws_floats"][0] is _lib.SIGNATURES["rsu_head_w_ws_floats"][0]
    assert len(_lib.SIGNATURES["rsu_head_dice_sums"][1]) == 11
    assert len(_lib.SIGNATURES["rsu_head_fwd_bwd_dice"][1]) == 20
    # the contract of the buffer between the two launches is written where a host integrator reads it
    for phrase in ("dice_sums", "no host synchronisation", "OVERWRITES"):
        assert phrase in header, phrase


def test_library_exports_the_dice_entry_points_and_sizes_the_workspace():
    L = _lib.lib()
    for s in NEW_SYMBOLS:
        assert hasattr(L, s), s
    for npix, C in ((3 * 37 * 41, 64), (3 * 37 * 41, 16), (4 * 388 * 388, 64), (1, 8)):
        n = L.rsu_head_dice_ws_floats(npix, C)
        assert n >= L.rsu_head_w_ws_floats(npix, C) and n >= 3     # enough for either call
