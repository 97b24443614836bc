"""No GPU: the fifth public header include/rsu_lovasz.h (the Lovasz term). The library exports what the header declares and
_lib.SIGNATURES_LOVASZ binds exactly that, disjoint from the other four tables, which did not grow; the size function and the refusals;
tests/test_gpu_lovasz_fenced.py leaves no launching entry of the header out (the rule of tests/test_cldice_host.py); the flag, its parser
and the UNet property; hostio.lovasz_loss / lovasz_gradient against the float64 torch statement of tests/lovasz_util.py where no two
errors tie, and on cases worked out by hand."""
import inspect
import os
import re

import numpy as np
import pytest

from road_segmentation_unet_amd import _lib, hostio
from road_segmentation_unet_amd import model as M
from road_segmentation_unet_amd.cli import parse_options
from road_segmentation_unet_amd.unet import UNet
from tests import lovasz_util as LU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
ENTRIES = ["rsu_lovasz_fwd", "rsu_lovasz_fwd_bwd", "rsu_lovasz_ws_bytes"]
LAUNCHING = ["rsu_lovasz_fwd", "rsu_lovasz_fwd_bwd"]


def _header(name):
    txt = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)


def _symbols(name):
    return sorted(set(re.findall(r"\b(rsu_[a-zA-Z0-9_]+)\s*\(", _header(name))))


# ------------------------------------------------------------------------------------------- ABI
def test_library_exports_the_fifth_header_and_the_table_binds_it():
    L = _lib.lib()
    syms = _symbols("rsu_lovasz.h")
    assert syms == ENTRIES
    for s in syms:
        assert hasattr(L, s), "librsu_hip.so does not export %s" % s
        assert getattr(L, s).argtypes == _lib.SIGNATURES_LOVASZ[s][1] and getattr(L, s).restype is _lib.SIGNATURES_LOVASZ[s][0]
    assert sorted(_lib.SIGNATURES_LOVASZ) == syms, "ctypes table and rsu_lovasz.h out of sync"
    tables = [set(_lib.SIGNATURES), set(_lib.SIGNATURES_OPTIM), set(_lib.SIGNATURES_LOSS), set(_lib.SIGNATURES_CLDICE), set(_lib.SIGNATURES_LOVASZ)]
    for i in range(5):
        for j in range(i + 1, 5):
            assert not (tables[i] & tables[j]), (i, j)
    # the other four headers declare what they did: the new entries live in the fifth
    assert sorted(_lib.SIGNATURES) == _symbols("rsu.h") and sorted(_lib.SIGNATURES_OPTIM) == _symbols("rsu_optim.h")
    assert sorted(_lib.SIGNATURES_LOSS) == _symbols("rsu_loss.h") == ["rsu_head_eval_focal", "rsu_head_fwd_bwd_focal"]
    assert sorted(_lib.SIGNATURES_CLDICE) == _symbols("rsu_cldice.h") == ["rsu_cldice_bwd", "rsu_cldice_fwd", "rsu_cldice_ws_floats", "rsu_head_fwd_bwd_aux"]
    assert not [n for h in ("rsu.h", "rsu_optim.h", "rsu_loss.h", "rsu_cldice.h") for n in _symbols(h) if "lovasz" in n]
    text = _header("rsu_lovasz.h")
    assert '#include "rsu.h"' in text
    # the argument lists of the header and of the table: the same lengths, floats (by value) and longs / ints in the same positions
    protos = re.findall(r"^(int|size_t) (rsu_\w+)\(([^;]*?)\);", text, flags=re.M | re.S)
    assert sorted(n for _, n, _ in protos) == ENTRIES
    for ret, name, args in protos:
        kinds = []
        for a in args.split(","):
            a = " ".join(a.split())
            kinds.append("f" if re.fullmatch(r"float \w+", a) else "l" if re.fullmatch(r"long \w+", a) else "i" if re.fullmatch(r"int \w+", a) else "p")
            assert kinds[-1] != "p" or "*" in a or a.startswith("rsu_stream_t "), (name, a)
        table = ["f" if t is _lib._f else "l" if t is _lib._l else "i" if t is _lib._i else "p" for t in _lib.SIGNATURES_LOVASZ[name][1]]
        assert kinds == table, (name, kinds, table)
        assert _lib.SIGNATURES_LOVASZ[name][0] is (_lib._sz if ret == "size_t" else _lib._i)


def _ws_formula(B, H, W):
    """rsu_lovasz.h: B * Pn keys of 8 bytes, and per tile of 4096 keys two int32 counts and one float sum"""
    pn = 4096
    while pn < H * W:
        pn *= 2
    return B * pn * 8 + B * pn // 4096 * 12


def test_size_function_and_refusals_without_a_gpu():
    L = _lib.lib()
    for shape in ((3, 37, 41), (1, 1, 1), (4, 388, 388), (1, 64, 64), (1, 64, 65), (1, 4096, 4096), (127, 4096, 4096)):
        assert L.rsu_lovasz_ws_bytes(*shape) == _ws_formula(*shape), shape
    assert _ws_formula(4, 388, 388) == 4 * (1 << 18) * 8 + 4 * 64 * 12
    for bad in ((0, 5, 5), (5, 0, 5), (5, 5, 0), (-1, 5, 5), (1, 4096, 4097), (1, 1 << 13, 1 << 12), (128, 4096, 4096), (1 << 30, 2, 1)):
        assert L.rsu_lovasz_ws_bytes(*bad) == 0, bad
    # refused before anything is launched: NULL pointers never reach a device
    assert L.rsu_lovasz_fwd(None, None, None, None, 1, 5, 5, None) == -22
    assert L.rsu_lovasz_fwd_bwd(None, None, 1.0, 0, None, None, None, 1, 5, 5, None) == -22


def test_the_fenced_file_covers_every_launching_entry_of_the_fifth_header():
    """tests/test_cldice_host.py's rule for rsu_cldice.h, for rsu_lovasz.h and tests/test_gpu_lovasz_fenced.py"""
    from tests import test_gpu_lovasz_fenced as G
    protos = re.findall(r"^(int|size_t) (rsu_\w+)\(([^;]*?)\);", _header("rsu_lovasz.h"), flags=re.M | re.S)
    launching = [n for r, n, a in protos if r == "int" and "rsu_stream_t" in a]
    assert sorted(launching) == LAUNCHING and [n for r, n, a in protos if r == "size_t"] == ["rsu_lovasz_ws_bytes"]
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
    assert "rsu_lovasz_ws_bytes" in inspect.getsource(G)   # exact workspaces


# ------------------------------------------------------------------------------------------- the flag, its parser, the property
def test_flag_and_parser():
    assert M.parse_lovasz_weight(0) == 0.0 and M.parse_lovasz_weight("1.5") == 1.5 and isinstance(M.parse_lovasz_weight(np.float32(2)), float)
    for bad in (-1e-3, float("nan"), float("inf"), "x", "", None, True, (1, 2)):
        with pytest.raises(ValueError):
            M.parse_lovasz_weight(bad)
    for o in (M.Options(), parse_options([])):
        assert o.lovasz_weight == 0.0 and isinstance(o.lovasz_weight, float)
    assert parse_options(["--lovasz_weight=1"]).lovasz_weight == 1.0 and M.Options(lovasz_weight="0.5").lovasz_weight == 0.5
    for bad in ("--lovasz_weight=-1", "--lovasz_weight=nan", "--lovasz_weight=inf"):
        with pytest.raises(ValueError):
            parse_options([bad])
    with pytest.raises(SystemExit):
        parse_options(["--lovasz_weight=one"])
    defs = {d[0]: d for d in M.EXTRA_FLAG_DEFS}
    assert defs["lovasz_weight"][1:3] == (float, 0.0)
    text = " ".join(defs["lovasz_weight"][3].split())
    for needle in ("0 = off", "1 - IoU", "per-image", "Ignored pixels add nothing", "do not enter it"):
        assert needle in text, needle


def test_unet_property_rejects_without_a_device():
    class Host:   # the UNet property on the attribute it keeps
        lovasz_weight = UNet.lovasz_weight
    h = Host()
    h.lovasz_weight = "0.5"
    assert h.lovasz_weight == 0.5
    for bad in (-0.5, float("nan"), float("inf"), "x", None):
        with pytest.raises(_lib.RsuError):
            h.lovasz_weight = bad
    assert h.lovasz_weight == 0.5
    assert inspect.signature(UNet.__init__).parameters["lovasz_weight"].default == 0.0
    assert inspect.signature(UNet.backward_device).parameters["lovasz_scale"].default is None
    with pytest.raises(_lib.RsuError, match="forward-only"):   # refused in front of any device work, as with cldice_weight
        UNet(2, 16, False, 2, 20, device="cpu", training=False, lovasz_weight=1.0)


# ------------------------------------------------------------------------------------------- the mirror against the float64 statement
@pytest.mark.parametrize("shape", [(3, 37, 41), (2, 5, 3), (1, 1, 1), (1, 64, 65), (2, 100, 100)])
def test_mirror_against_the_float64_statement_where_nothing_ties(shape):
    p, labels = LU.tie_free(shape)
    B, n = shape[0], shape[1] * shape[2]
    for b in range(B):
        e = np.abs(labels[b].astype(f32) - p[b]).reshape(-1)
        assert len(np.unique(e.view(np.uint32))) == n          # tie-free by construction
    losses = hostio.lovasz_loss(p, labels)
    g = hostio.lovasz_gradient(p, labels, LU.SCALE)
    assert losses.dtype == f32 and losses.shape == (B,) and g.dtype == f32 and g.shape == p.shape
    ref_losses, ref_g = LU.torch_lovasz(p, labels, LU.SCALE)
    # every g_k: q = I / U <= 1 carries one rounding (<= u), J = 1 - q a second (<= 2 u in all), g = J_k - J_{k-1} a third (<= 2 u + 2 u + u);
    # f32(scale), c = scale / B and c * g carry one relative u each: |g32 - g64| <= c (5 u + 3 u |g|) <= 8 u c, all values in [0, 1]
    c = LU.SCALE / B
    err_g = float(np.abs(g.astype(np.float64) - ref_g).max())
    print("lovasz mirror %s: max |g32 - g64| = %.3g = %.2f u c" % (shape, err_g, err_g / (LU.U32 * c)))
    assert err_g <= 8 * LU.U32 * c
    # the loss: a term e_k g_k is off by at most 5 u e_k + 2 u e_k g_k (g as above; e = |y - p| and the product one rounding each), and
    # the float32 sum of the n terms by numpy's pairwise bound
    for b in range(B):
        e = np.abs(labels[b].astype(np.float64) - p[b].astype(np.float64)).sum()
        bound = 5 * LU.U32 * e + 2 * LU.U32 * ref_losses[b] + LU.sum_bound(LU.host_depth(n), ref_losses[b]) + LU.U32 * ref_losses[b]
        err = abs(float(losses[b]) - ref_losses[b])
        print("  image %d: L = %.7f, |L32 - L64| = %.3g, bound %.3g" % (b, ref_losses[b], err, bound))
        assert err <= bound
    assert (g != 0).mean() > 0.5


# ------------------------------------------------------------------------------------------- pinned cases, by hand
def test_nothing_counted_gives_zeros():
    p = np.full((2, 3, 4), 0.3, f32)
    labels = np.full((2, 3, 4), -1, np.int64)
    labels[1, 0, 0] = 1 << 32
    assert not hostio.lovasz_loss(p, labels).any()
    g = hostio.lovasz_gradient(p, labels, 1.0)
    assert not g.any() and not np.signbit(g).any()


def test_empty_ground_truth_is_the_largest_error():
    p = np.array([[[0.2, 0.9, 0.1], [0.9, 0.5, 0.9]]], f32)
    labels = np.zeros((1, 2, 3), np.int64)
    assert hostio.lovasz_loss(p, labels)[0] == f32(0.9)
    g = hostio.lovasz_gradient(p, labels, 1.0)
    want = np.zeros((1, 2, 3), f32)
    want[0, 0, 1] = 1.0                      # the FIRST pixel of largest p
    assert np.array_equal(g, want)


def test_all_road_by_hand():
    """G = n = 3: ranks by e = 1 - p descending; c_k = k, I_k = 3 - k, U_k = 3: J = 1/3, 2/3, 1 and every g_k is 1/3 as float32 rounds it"""
    p = np.array([[[0.75, 0.25, 0.5]]], f32)
    labels = np.ones((1, 1, 3), np.int64)
    J = [f32(1) - f32(2) / f32(3), f32(1) - f32(1) / f32(3), f32(1) - f32(0) / f32(3)]
    gk = [J[0], J[1] - J[0], J[2] - J[1]]
    es = [f32(0.75), f32(0.5), f32(0.25)]        # pixel 1, pixel 2, pixel 0
    want_loss = np.sum(np.array([es[i] * gk[i] for i in range(3)], f32), dtype=f32)
    assert hostio.lovasz_loss(p, labels)[0] == want_loss and abs(float(want_loss) - 0.5) < 1e-6
    g = hostio.lovasz_gradient(p, labels, 2.0)
    assert np.array_equal(g, np.array([[[-(f32(2) * gk[2]), -(f32(2) * gk[0]), -(f32(2) * gk[1])]]], f32))


def test_all_p_equal_ranks_by_pixel_index():
    """y = 0 everywhere and one p: every error ties, so rank k is pixel k - 1 and only the first pixel gets a gradient (G = 0)"""
    p = np.full((1, 3, 5), 0.25, f32)
    g = hostio.lovasz_gradient(p, np.zeros((1, 3, 5), np.int64), 1.0)
    assert g.reshape(-1)[0] == 1.0 and not g.reshape(-1)[1:].any()
    # with labels the errors differ by class only: e = 0.75 for y = 1 first, in index order, then e = 0.25 for y = 0 in index order
    labels = np.array([[[0, 1, 0, 1, 0]]], np.int64)
    p = np.full((1, 1, 5), 0.25, f32)
    g = hostio.lovasz_gradient(p, labels, 1.0).reshape(-1)
    # ranks: pixel 1, pixel 3, then 0, 2, 4. G = 2: J = 1 - 1/2, 1 - 0/2, 1, 1, 1
    assert np.array_equal(g, np.array([0.0, -0.5, 0.0, -0.5, 0.0], f32))
    assert hostio.lovasz_loss(p, labels)[0] == f32(0.75)


def test_two_by_three_by_hand():
    """labels 1 0 0 / 1 0 -1, p .5 .75 .25 / .75 .75 .9: errors .5 .75 .25 / .25 .75 (ignored). Ranks: (0,1) and (1,1) tie at .75 -> index
    order; then (0,0) at .5; then (0,2) and (1,0) tie at .25 -> index order. y along the ranks: 0 0 1 0 1, G = 2."""
    p = np.array([[[0.5, 0.75, 0.25], [0.75, 0.75, 0.9]]], f32)
    labels = np.array([[[1, 0, 0], [1, 0, -1]]], np.int64)
    one = f32(1)
    #   k      1        2        3        4        5
    #   c      0        0        1        1        2
    #   I      2        2        1        1        0
    #   U      3        4        4        5        5
    J = [one - f32(2) / f32(3), one - f32(2) / f32(4), one - f32(1) / f32(4), one - f32(1) / f32(5), one - f32(0) / f32(5)]
    gk = [J[0]] + [J[i] - J[i - 1] for i in range(1, 5)]
    es = [f32(0.75), f32(0.75), f32(0.5), f32(0.25), f32(0.25)]
    want_loss = np.sum(np.array([es[i] * gk[i] for i in range(5)], f32), dtype=f32)
    assert hostio.lovasz_loss(p, labels)[0] == want_loss
    c = f32(0.5) / f32(1)
    want = np.array([[[-(c * gk[2]), c * gk[0], c * gk[3]], [-(c * gk[4]), c * gk[1], 0.0]]], f32)
    got = hostio.lovasz_gradient(p, labels, 0.5)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    # `into`: added with one rounding, the argument untouched
    base = np.full((1, 2, 3), 0.125, f32)
    assert np.array_equal(hostio.lovasz_gradient(p, labels, 0.5, into=base), base + want) and np.all(base == 0.125)


def test_mirror_refuses():
    z = np.zeros((1, 4, 4), f32)
    with pytest.raises(ValueError):
        hostio.lovasz_loss(np.zeros((4, 4), f32), np.zeros((4, 4), np.int64))
    with pytest.raises(ValueError):
        hostio.lovasz_gradient(z, np.zeros((1, 4, 5), np.int64), 1.0)
    for scale in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            hostio.lovasz_gradient(z, np.zeros((1, 4, 4), np.int64), scale)
    with pytest.raises(ValueError):
        hostio.lovasz_gradient(z, np.zeros((1, 4, 4), np.int64), 1.0, into=np.zeros((1, 4, 5), f32))
