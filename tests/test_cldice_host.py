"""No GPU: the fourth public header include/rsu_cldice.h (the clDice term). The library exports what the header declares and
_lib.SIGNATURES_CLDICE binds exactly that, disjoint from the other three tables, which did not grow; tests/test_gpu_cldice_fenced.py leaves
no launching entry of the header out (the rule of tests/test_focal_host.py); the flags, their parsers and the UNet properties;
hostio.soft_skeleton against the torch restatement of the published soft_skel, its float32 and float64 decisions; hostio.cldice_gradient
against torch float64 autograd where no window has a tie, and apart from it where windows do; a line, a constant image."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from road_segmentation_unet_amd import _lib, hostio
from road_segmentation_unet_amd import model as M
from road_segmentation_unet_amd.cli import parse_options
from road_segmentation_unet_amd.unet import UNet
from tests import cldice_util as CU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
ENTRIES = ["rsu_cldice_bwd", "rsu_cldice_fwd", "rsu_cldice_ws_floats", "rsu_head_fwd_bwd_aux"]
LAUNCHING = ["rsu_cldice_bwd", "rsu_cldice_fwd", "rsu_head_fwd_bwd_aux"]


def _header(name):
    txt = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)


def _symbols(name):
    return sorted(set(re.findall(r"\b(rsu_[a-zA-Z0-9_]+)\s*\(", _header(name))))


# ------------------------------------------------------------------------------------------- ABI
def test_library_exports_the_fourth_header_and_the_table_binds_it():
    L = _lib.lib()
    syms = _symbols("rsu_cldice.h")
    assert syms == ENTRIES
    for s in syms:
        assert hasattr(L, s), "librsu_hip.so does not export %s" % s
        assert getattr(L, s).argtypes == _lib.SIGNATURES_CLDICE[s][1] and getattr(L, s).restype is _lib.SIGNATURES_CLDICE[s][0]
    assert sorted(_lib.SIGNATURES_CLDICE) == syms, "ctypes table and rsu_cldice.h out of sync"
    tables = [set(_lib.SIGNATURES), set(_lib.SIGNATURES_OPTIM), set(_lib.SIGNATURES_LOSS), set(_lib.SIGNATURES_CLDICE)]
    for i in range(4):
        for j in range(i + 1, 4):
            assert not (tables[i] & tables[j]), (i, j)
    # the other three headers did not grow: the new entries live in the fourth
    assert sorted(_lib.SIGNATURES) == _symbols("rsu.h") and sorted(_lib.SIGNATURES_OPTIM) == _symbols("rsu_optim.h")
    assert sorted(_lib.SIGNATURES_LOSS) == _symbols("rsu_loss.h") == ["rsu_head_eval_focal", "rsu_head_fwd_bwd_focal"]
    assert not [n for n in _symbols("rsu.h") + _symbols("rsu_optim.h") + _symbols("rsu_loss.h") if "cldice" in n or "aux" in n]
    text = _header("rsu_cldice.h")
    assert '#include "rsu.h"' in text and re.search(r"#define RSU_CLDICE_MAX_ITERS 16\b", text)
    assert _lib.CLDICE_MAX_ITERS == 16 == hostio.CLDICE_MAX_ITERS
    # the argument lists of the header and of the table: the same lengths, floats (by value) and longs / ints in the same positions
    protos = re.findall(r"^(int|size_t) (rsu_\w+)\(([^;]*?)\);", text, flags=re.M | re.S)
    assert sorted(n for _, n, _ in protos) == ENTRIES
    for ret, name, args in protos:
        kinds = []
        for a in args.split(","):
            a = " ".join(a.split())
            kinds.append("f" if re.fullmatch(r"float \w+", a) else "l" if re.fullmatch(r"long \w+", a) else "i" if re.fullmatch(r"int \w+", a) else "p")
            assert kinds[-1] != "p" or "*" in a or a.startswith("rsu_stream_t "), (name, a)
        table = ["f" if t is _lib._f else "l" if t is _lib._l else "i" if t is _lib._i else "p" for t in _lib.SIGNATURES_CLDICE[name][1]]
        assert kinds == table, (name, kinds, table)
        assert _lib.SIGNATURES_CLDICE[name][0] is (_lib._sz if ret == "size_t" else _lib._i)
    # rsu_head_fwd_bwd_aux is rsu_head_fwd_bwd_focal's list with gprob in front of the stream
    focal, aux = _lib.SIGNATURES_LOSS["rsu_head_fwd_bwd_focal"][1], _lib.SIGNATURES_CLDICE["rsu_head_fwd_bwd_aux"][1]
    assert aux == focal[:-1] + [_lib._vp] + focal[-1:]


def test_size_function_and_refusals_without_a_gpu():
    L = _lib.lib()
    for B, H, W, k in ((3, 37, 41, 3), (1, 1, 1, 0), (4, 388, 388, 16)):
        n, tiles = B * H * W, B * (-(-H // 32)) * (-(-W // 32))
        assert L.rsu_cldice_ws_floats(B, H, W, k) == (2 * k + 1) * n + 4 * tiles
    for bad in ((0, 5, 5, 3), (5, 0, 5, 3), (5, 5, 0, 3), (5, 5, 5, -1), (5, 5, 5, 17), (1 << 11, 1 << 10, 1 << 10, 3)):
        assert L.rsu_cldice_ws_floats(*bad) == 0, bad
    # refused before anything is launched: NULL pointers never reach a device
    assert L.rsu_cldice_fwd(None, None, 3, None, None, None, None, 1, 5, 5, None) == -22
    assert L.rsu_cldice_bwd(None, None, None, None, None, 3, 1.0, 1.0, None, None, 1, 5, 5, None) == -22


def test_the_fenced_file_covers_every_launching_entry_of_the_fourth_header():
    """tests/test_focal_host.py's rule for rsu_loss.h, for rsu_cldice.h and tests/test_gpu_cldice_fenced.py"""
    from tests import test_gpu_cldice_fenced as G
    protos = re.findall(r"^(int|size_t) (rsu_\w+)\(([^;]*?)\);", _header("rsu_cldice.h"), flags=re.M | re.S)
    launching = [n for r, n, a in protos if r == "int" and "rsu_stream_t" in a]
    assert sorted(launching) == LAUNCHING and [n for r, n, a in protos if r == "size_t"] == ["rsu_cldice_ws_floats"]
    tests = {n: f for n, f in vars(G).items() if n.startswith("test_") and callable(f)}
    for entry in launching:
        assert (entry in G.FENCED) != (entry in G.NOT_FENCED), "%s: in exactly one of FENCED and NOT_FENCED" % entry
    assert set(G.FENCED) | set(G.NOT_FENCED) <= set(launching)
    for entry, names in G.FENCED.items():
        assert names, entry
        for n in names:
            assert n in tests, (entry, n)
            assert re.search(r'"%s"' % entry, inspect.getsource(tests[n]) + "".join(inspect.getsource(h) for h in G.HELPERS.get(n, ()))), \
                "%s is not launched by %s" % (entry, n)
    for entry, reason in G.NOT_FENCED.items():
        assert "writes no device memory" in reason, (entry, reason)
    assert "pytest.mark.gpu" in inspect.getsource(G)
    assert "rsu_cldice_ws_floats" in inspect.getsource(G) and "rsu_head_dice_ws_floats" in inspect.getsource(G)   # exact workspaces


# ------------------------------------------------------------------------------------------- flags, parsers, properties
def test_flags_and_parsers():
    assert M.parse_cldice_weight(0) == 0.0 and M.parse_cldice_weight("1.5") == 1.5 and isinstance(M.parse_cldice_weight(np.float32(2)), float)
    assert M.parse_cldice_smooth("0.5") == 0.5 and M.parse_cldice_smooth(2) == 2.0
    assert M.parse_cldice_iters(0) == 0 and M.parse_cldice_iters("16") == 16 and M.parse_cldice_iters(np.int64(7)) == 7
    for bad in (-1e-3, float("nan"), float("inf"), "x", "", None, True, (1, 2)):
        with pytest.raises(ValueError):
            M.parse_cldice_weight(bad)
    for bad in (0, -1.0, float("nan"), float("inf"), "x", None, True):
        with pytest.raises(ValueError):
            M.parse_cldice_smooth(bad)
    for bad in (-1, 17, 2.5, "x", "", None, True, float("nan"), (3,)):
        with pytest.raises(ValueError):
            M.parse_cldice_iters(bad)
    for o in (M.Options(), parse_options([])):
        assert (o.cldice_weight, o.cldice_iters, o.cldice_smooth) == (0.0, 10, 1.0)
        assert isinstance(o.cldice_weight, float) and isinstance(o.cldice_iters, int)
    o = parse_options(["--cldice_weight=1", "--cldice_iters", "3", "--cldice_smooth=0.5"])
    assert (o.cldice_weight, o.cldice_iters, o.cldice_smooth) == (1.0, 3, 0.5)
    assert M.Options(cldice_iters="4").cldice_iters == 4
    for bad in ("--cldice_weight=-1", "--cldice_weight=nan", "--cldice_iters=17", "--cldice_iters=-1", "--cldice_smooth=0", "--cldice_smooth=inf"):
        with pytest.raises(ValueError):
            parse_options([bad])
    for bad in ("--cldice_weight=one", "--cldice_iters=2.5"):
        with pytest.raises(SystemExit):
            parse_options([bad])
    defs = {d[0]: d for d in M.EXTRA_FLAG_DEFS}
    assert defs["cldice_weight"][1:3] == (float, 0.0) and defs["cldice_iters"][1:3] == (int, 10) and defs["cldice_smooth"][1:3] == (float, 1.0)
    text = " ".join(defs["cldice_weight"][3].split())
    for needle in ("0 = off", "connectivity", "Ignored pixels add nothing", "do not enter it"):
        assert needle in text, needle


def test_unet_properties_reject_without_a_device():
    class Host:   # the UNet properties on the attributes they keep
        cldice_weight, cldice_iters, cldice_smooth = UNet.cldice_weight, UNet.cldice_iters, UNet.cldice_smooth
    h = Host()
    h.cldice_weight, h.cldice_iters, h.cldice_smooth = "0.5", 3, 2
    assert (h.cldice_weight, h.cldice_iters, h.cldice_smooth) == (0.5, 3, 2.0)
    for name, bads in (("cldice_weight", (-0.5, float("nan"), float("inf"), "x", None)), ("cldice_iters", (-1, 17, 2.5, "3", None, True)),
                       ("cldice_smooth", (0.0, -1, float("nan"), float("inf"), "x", None))):
        for bad in bads:
            with pytest.raises(_lib.RsuError):
                setattr(h, name, bad)
    assert (h.cldice_weight, h.cldice_iters, h.cldice_smooth) == (0.5, 3, 2.0)
    sig = inspect.signature(UNet.__init__).parameters
    assert (sig["cldice_weight"].default, sig["cldice_iters"].default, sig["cldice_smooth"].default) == (0.0, 10, 1.0)
    assert inspect.signature(UNet.backward_device).parameters["cldice_scale"].default is None


def test_cldice_from_sums_is_plain_arithmetic():
    assert M.cldice_from_sums(0.0, 0.0, 0.0, 0.0, 1.0) == 1.0
    A, Bp, Cc, Dy, s = 3.0, 11.0, 5.0, 7.0, 0.5
    Tp, Ts = (A + s) / (Bp + s), (Cc + s) / (Dy + s)
    assert M.cldice_from_sums(A, Bp, Cc, Dy, s) == pytest.approx(2 * Tp * Ts / (Tp + Ts), rel=1e-15)
    t = M.cldice_from_sums(*(torch.tensor([v], dtype=torch.float64) for v in (A, Bp, Cc, Dy)), s)
    assert isinstance(t, torch.Tensor) and float(t) == pytest.approx(2 * Tp * Ts / (Tp + Ts), rel=1e-15)
    assert M.cldice_from_sums(np.array([A]), np.array([Bp]), np.array([Cc]), np.array([Dy]), s).shape == (1,)


# ------------------------------------------------------------------------------------------- soft_skeleton
HOST_CASES = [((3, 37, 41), 3), ((2, 40, 40), 10), ((1, 5, 3), 16), ((1, 1, 1), 3), ((2, 1, 40), 3), ((2, 40, 1), 16), ((3, 37, 41), 0)]


@pytest.mark.parametrize("shape,iters", HOST_CASES)
@pytest.mark.parametrize("kind", sorted(CU.INPUTS))
def test_soft_skeleton_against_the_torch_restatement(shape, iters, kind):
    p, _ = CU.INPUTS[kind](shape)
    got = hostio.soft_skeleton(p, iters)
    assert got.dtype == np.float32 and got.shape == p.shape
    ref32 = CU.torch_skeleton(torch.tensor(p), iters).numpy()
    ref64 = CU.torch_skeleton(torch.tensor(p, dtype=torch.float64), iters).numpy()
    err = float(np.abs(got.astype(np.float64) - ref64).max())
    print("soft_skeleton %s k=%d %s: max error against float64 %.3g; equal to torch float32: %s" % (shape, iters, kind, err, np.array_equal(got, ref32)))
    assert err <= 1e-6
    # the decisions of the float32 and of the float64 run are identical: what lets a float64 reference check a float32 kernel at all
    c32, c64 = hostio._cldice_chain(p, iters), hostio._cldice_chain(p.astype(np.float64), iters)
    for j in range(iters + 1):
        assert np.array_equal(c32[1][j], c64[1][j]) and np.array_equal(c32[2][j], c64[2][j]), j        # the winners of both windows
        assert np.array_equal(c32[3][j] > 0, c64[3][j] > 0), j                                           # the first ReLU
        if j:
            assert np.array_equal(c32[5][j], c64[5][j]), j                                               # the second


def test_soft_skeleton_refuses():
    for bad in (-1, 17, 2.5, True):
        with pytest.raises(ValueError):
            hostio.soft_skeleton(np.zeros((1, 4, 4), f32), bad)
    with pytest.raises(ValueError):
        hostio.soft_skeleton(np.zeros((4, 4), f32), 3)
    with pytest.raises(ValueError):
        hostio.cldice_gradient(np.zeros((1, 4, 4), f32), np.zeros((1, 4, 5), np.int64), 3, 1.0, 1.0)
    for scale, smooth in ((-1.0, 1.0), (float("nan"), 1.0), (1.0, 0.0), (1.0, float("inf"))):
        with pytest.raises(ValueError):
            hostio.cldice_gradient(np.zeros((1, 4, 4), f32), np.zeros((1, 4, 4), np.int64), 3, scale, smooth)


# ------------------------------------------------------------------------------------------- cldice_gradient
@pytest.mark.parametrize("shape,iters", HOST_CASES)
def test_gradient_against_torch_autograd_where_nothing_ties(shape, iters):
    p, labels = CU.tie_free(shape)
    sp, sy, sums, g = hostio.cldice_gradient(p, labels, iters, CU.SCALE, CU.SMOOTH)
    rsp, rsy, rsums, rg, _ = CU.torch_cldice(p, labels, iters, CU.SCALE, CU.SMOOTH)
    err = float(np.abs(g - rg).max())
    print("cldice_gradient %s k=%d: max |g - autograd| %.3g at max |g| %.3g" % (shape, iters, err, float(np.abs(rg).max())))
    assert err <= 1e-12 and np.abs(sp - rsp).max() <= 1e-12 and np.abs(sy - rsy).max() <= 1e-12
    assert np.all(np.abs(sums - rsums) <= 1e-12 * np.maximum(1.0, np.abs(rsums)))
    ign = (labels != 0) & (labels != 1)
    assert not g[ign].any()


@pytest.mark.parametrize("lev", [4, 8, 16])
def test_gradient_pins_its_own_tie_rule(lev):
    """on quantised maps torch.min(p1, p2) splits the ties of the cross in halves: the two sub-gradients differ at more than a tenth of the
    pixels, so a test against hostio.cldice_gradient sees which rule a kernel follows. The values do not depend on the rule."""
    shape, iters = (3, 37, 41), 3
    p, labels = CU.tied(shape, lev, ignored=False)
    sp, sy, sums, g = hostio.cldice_gradient(p, labels, iters, CU.SCALE, CU.SMOOTH)
    rsp, _, rsums, rg, _ = CU.torch_cldice(p, labels, iters, CU.SCALE, CU.SMOOTH)
    assert np.abs(sp - rsp).max() <= 1e-12 and np.all(np.abs(sums - rsums) <= 1e-9)
    differ = float((np.abs(g - rg) > 1e-9 * np.abs(rg).max()).mean())
    print("lev %d: the rules differ at %.1f %% of the pixels, by up to %.2f of max |g|" % (lev, 100 * differ, np.abs(g - rg).max() / np.abs(rg).max()))
    assert differ > 0.10
    assert abs(g.sum() - rg.sum()) <= 1e-9 * np.abs(rg).sum()       # both rules conserve the gradient's sum


def test_given_sums_change_the_factors_only():
    p, labels = CU.tie_free((2, 9, 11))
    a = hostio.cldice_gradient(p, labels, 3, 1.0, 1.0)
    b = hostio.cldice_gradient(p, labels, 3, 1.0, 1.0, sums=a[2])
    c = hostio.cldice_gradient(p, labels, 3, 1.0, 1.0, sums=[3.0, 11.0, 5.0, 7.0])
    assert np.array_equal(a[3], b[3]) and np.array_equal(a[2], c[2]) and not np.allclose(a[3], c[3])


# ------------------------------------------------------------------------------------------- properties
def test_a_line_is_its_own_skeleton_and_a_constant_image_has_none():
    line = np.zeros((1, 9, 13), f32)
    line[0, 4, :] = 1.0
    for k in (0, 1, 3, 16):
        assert np.array_equal(hostio.soft_skeleton(line, k), line), k
    const = np.full((2, 7, 9), 0.37, f32)
    assert not hostio.soft_skeleton(const, 5).any()
    labels = np.ones((2, 7, 9), np.int64)
    sp, sy, sums, g = hostio.cldice_gradient(const, labels, 5, 1.0, 1.0)
    assert not sums.any() and float(M.cldice_from_sums(*sums, 1.0)) == 1.0 and not g.any()
