"""No GPU: the eighth public header include/rsu_thin.h (centre-lines). The library exports what the header declares and _lib.SIGNATURES_THIN
binds exactly that, disjoint from the other seven tables; the size function and every refusal with NULL device pointers; the 2-GiB
refusal one image past the limit; tests/test_gpu_thin_fenced.py leaves no launching entry of the header out; the flags, their parsers
and refusals; hostio.thin_mask held to the topology of its input over the bank of tests/thin_util.py (subset, the same 8-connected
foreground and 4-connected background components by scipy, idempotent; truncated runs too); mask_thin's formats and counts;
centerline_metrics on hand-counted cases."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from road_segmentation_unet_amd import _lib, hostio
from road_segmentation_unet_amd import model as M
from road_segmentation_unet_amd.cli import parse_options
from tests import thin_util as TU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["rsu_mask_thin", "rsu_thin_ws_bytes"]
LAUNCHING = ["rsu_mask_thin"]
EINVAL = -22
p = ctypes.c_void_p(0x1000)   # a pointer no refused call may follow


def _header(name):
    txt = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)


def _symbols(name):
    return sorted(set(re.findall(r"\b(rsu_[a-zA-Z0-9_]+)\s*\(", _header(name))))


def _protos(name):
    return re.findall(r"^(int|size_t) (rsu_\w+)\(([^;]*?)\);", _header(name), flags=re.M | re.S)


# ------------------------------------------------------------------------------------------- ABI
def test_library_exports_the_eighth_header_and_the_table_binds_it():
    L = _lib.lib()
    syms = _symbols("rsu_thin.h")
    assert syms == ENTRIES
    for s in syms:
        assert hasattr(L, s), "librsu_hip.so does not export %s" % s
        assert getattr(L, s).argtypes == _lib.SIGNATURES_THIN[s][1] and getattr(L, s).restype is _lib.SIGNATURES_THIN[s][0]
    assert sorted(_lib.SIGNATURES_THIN) == syms, "ctypes table and rsu_thin.h out of sync"
    tables = [set(_lib.SIGNATURES), set(_lib.SIGNATURES_OPTIM), set(_lib.SIGNATURES_LOSS), set(_lib.SIGNATURES_CLDICE),
              set(_lib.SIGNATURES_LOVASZ), set(_lib.SIGNATURES_COMPONENTS), set(_lib.SIGNATURES_DISTANCE), set(_lib.SIGNATURES_THIN)]
    for i in range(8):
        for j in range(i + 1, 8):
            assert not (tables[i] & tables[j]), (i, j)
    others = ("rsu.h", "rsu_optim.h", "rsu_loss.h", "rsu_cldice.h", "rsu_lovasz.h", "rsu_components.h", "rsu_distance.h")
    assert not [n for h in others for n in _symbols(h) if "thin" in n]
    assert sorted(_lib.SIGNATURES_DISTANCE) == _symbols("rsu_distance.h")   # the seventh declares what it did
    assert '#include "rsu.h"' in _header("rsu_thin.h")
    for macro, value in (("RSU_THIN_MAX_SIDE", "1024"), ("RSU_THIN_MAX_ITERS", "512")):
        assert re.search(r"^#define %s %s$" % (macro, value), _header("rsu_thin.h"), flags=re.M), macro
    assert (_lib.THIN_MAX_SIDE, _lib.THIN_MAX_ITERS) == (1024, 512) == (hostio.THIN_MAX_SIDE, hostio.THIN_MAX_ITERS) == (TU.MAX_SIDE, TU.MAX_ITERS)
    # the argument lists of the header and of the table: the same lengths, floats (by value) and ints in the same positions
    protos = _protos("rsu_thin.h")
    assert sorted(n for _, n, _ in protos) == ENTRIES
    for ret, name, args in protos:
        kinds = []
        for a in args.split(","):
            a = " ".join(a.split())
            kinds.append("f" if re.fullmatch(r"float \w+", a) else "l" if re.fullmatch(r"long \w+", a) else "i" if re.fullmatch(r"int \w+", a) else "p")
            assert kinds[-1] != "p" or "*" in a or a.startswith("rsu_stream_t "), (name, a)
        table = ["f" if t is _lib._f else "l" if t is _lib._l else "i" if t is _lib._i else "p" for t in _lib.SIGNATURES_THIN[name][1]]
        assert kinds == table, (name, kinds, table)
        assert _lib.SIGNATURES_THIN[name][0] is (_lib._sz if ret == "size_t" else _lib._i)
    # the tile the test shapes are chosen for is the one the kernels are built with
    src = open(os.path.join(ROOT, "road_segmentation_unet_amd", "csrc", "thin.h")).read() + \
        open(os.path.join(ROOT, "road_segmentation_unet_amd", "csrc", "thin.hip")).read()
    assert re.search(r"^#define TH_K %d$" % TU.K, src, flags=re.M) and re.search(r"^#define TH_ROWS %d\b" % (TU.CROWS + 4 * TU.K), src, flags=re.M)
    assert TU.CORE == 64 - 4 * TU.K


def _ws(N, H, W, iters):
    """the layout of csrc/thin.hip: three bit planes of [N][2][H][ceil(W / CORE)] 64-bit words, then [ceil(iters / K) + 1][N][2] counters"""
    return 3 * N * 2 * H * (-(-W // TU.CORE)) * 8 + -(-((-(-iters // TU.K) + 1) * N * 2 * 4) // 8) * 8


def test_size_function_and_refusals_without_a_gpu():
    L = _lib.lib()
    for shape in TU.SHAPES + [(4, 388, 388), (2, 608, 608), (1, 1024, 1024), (255, 1024, 1024), (511, 1024, 1024)]:
        for iters in (1, 8, 9, 64, 512):
            need = L.rsu_thin_ws_bytes(*shape, iters)
            assert need == _ws(*shape, iters) and need % 8 == 0, (shape, iters)
    bad_sizes = ((0, 5, 5), (5, 0, 5), (5, 5, 0), (-1, 5, 5), (5, -1, 5), (5, 5, -1), (1, 1025, 5), (1, 5, 1025), (1, 1 << 20, 1))
    for bad in bad_sizes + ((512, 1024, 1024), (1 << 30, 2, 1)):
        assert L.rsu_thin_ws_bytes(*bad, 64) == 0, bad
    for iters in (0, -1, 513, 1 << 30):
        assert L.rsu_thin_ws_bytes(2, 5, 7, iters) == 0, iters
    # refused before anything is launched or dereferenced: NULL pointers, and pointers nobody may follow
    ok = (2, 5, 7)
    # prob, threshold, labels64, max_iters, skel_pred, skel_true, acc, info, ws
    assert L.rsu_mask_thin(None, 0.5, None, 64, None, None, None, None, None, *ok, None) == EINVAL
    assert L.rsu_mask_thin(None, 0.5, p, 64, p, p, p, p, p, *ok, None) == EINVAL         # prob
    assert L.rsu_mask_thin(p, 0.5, p, 64, p, p, p, p, None, *ok, None) == EINVAL         # ws
    assert L.rsu_mask_thin(p, 0.5, p, 64, None, None, None, p, p, *ok, None) == EINVAL   # both outputs
    assert L.rsu_mask_thin(p, 0.5, None, 64, p, p, None, p, p, *ok, None) == EINVAL      # skel_true without labels
    assert L.rsu_mask_thin(p, 0.5, None, 64, None, p, None, p, p, *ok, None) == EINVAL
    assert L.rsu_mask_thin(p, 0.5, p, 64, p, None, p, p, p, *ok, None) == EINVAL         # acc needs both skeletons
    assert L.rsu_mask_thin(p, 0.5, p, 64, None, p, p, p, p, *ok, None) == EINVAL
    assert L.rsu_mask_thin(p, 0.5, None, 64, p, None, p, p, p, *ok, None) == EINVAL
    for bad in bad_sizes:
        assert L.rsu_mask_thin(p, 0.5, p, 64, p, p, p, p, p, *bad, None) == EINVAL, bad
    for iters in (0, -1, 513, 1 << 30):
        assert L.rsu_mask_thin(p, 0.5, p, iters, p, p, p, p, p, *ok, None) == EINVAL, iters
    for t in (float("nan"), float("inf"), float("-inf")):
        assert L.rsu_mask_thin(p, t, p, 64, p, p, p, p, p, *ok, None) == EINVAL


def test_two_gib_refusal_one_image_past_the_limit():
    """at 1024 x 1024 labels64 and skel_true take 8 MiB per image: 255 images are the last batch below 0x7ffffff0 bytes, 256 reach 2 GiB.
    Without labels64 the largest tensor has 4 bytes per pixel: 511 images pass, 512 do not."""
    L = _lib.lib()
    S = 1024
    assert 255 * S * S * 8 < 0x7ffffff0 <= 256 * S * S * 8 and 511 * S * S * 4 < 0x7ffffff0 <= 512 * S * S * 4
    assert L.rsu_thin_ws_bytes(255, S, S, 64) == _ws(255, S, S, 64) > 0
    assert L.rsu_mask_thin(p, 0.5, p, 64, p, p, p, p, p, 256, S, S, None) == _lib.E2BIG
    assert L.rsu_mask_thin(p, 0.5, p, 64, None, p, None, None, p, 256, S, S, None) == _lib.E2BIG
    assert L.rsu_mask_thin(p, 0.5, p, 64, p, None, None, None, p, 256, S, S, None) == _lib.E2BIG    # labels64 given: it is the largest tensor
    assert L.rsu_mask_thin(p, 0.5, None, 64, p, None, None, None, p, 512, S, S, None) == _lib.E2BIG
    with pytest.raises(_lib.RsuError, match="2 GiB"):
        _lib.call("rsu_mask_thin", p, 0.5, p, 64, p, p, p, p, p, 256, S, S, None)
    # a wrong argument is reported before the size
    assert L.rsu_mask_thin(p, float("nan"), p, 64, p, p, p, p, p, 256, S, S, None) == EINVAL
    assert L.rsu_mask_thin(None, 0.5, p, 64, p, p, p, p, p, 256, S, S, None) == EINVAL
    assert L.rsu_mask_thin(p, 0.5, p, 0, p, p, p, p, p, 256, S, S, None) == EINVAL


def test_the_fenced_file_covers_every_launching_entry_of_the_eighth_header():
    from tests import test_gpu_thin_fenced as G
    protos = _protos("rsu_thin.h")
    launching = [n for r, n, a in protos if r == "int" and "rsu_stream_t" in a]
    assert sorted(launching) == LAUNCHING and [n for r, n, a in protos if r == "size_t"] == ["rsu_thin_ws_bytes"]
    tests = {n: f for n, f in vars(G).items() if n.startswith("test_") and callable(f)}
    assert sorted(G.FENCED) == LAUNCHING
    for entry, names in G.FENCED.items():
        assert names, entry
        for n in names:
            assert n in tests, (entry, n)
            assert re.search(r'"%s"' % entry, inspect.getsource(tests[n]) + "".join(inspect.getsource(h) for h in G.HELPERS.get(n, ()))), \
                "%s is not launched by %s" % (entry, n)
    assert "pytest.mark.gpu" in inspect.getsource(G)
    assert "rsu_thin_ws_bytes" in inspect.getsource(G)   # exact workspaces


# ------------------------------------------------------------------------------------------- the flags and their parsers
def test_flags_defaults_parsers_and_refusals():
    defs = {d[0]: d for d in M.EXTRA_FLAG_DEFS}
    assert defs["validate_centerlines"][1:3] == (bool, False) and defs["centerline_max_iters"][1:3] == (int, 64)
    assert defs["save_centerlines"][1:3] == (bool, False) and defs["save_best_metric"][1:3] == (str, "f1")
    for o in (M.Options(), parse_options([])):
        assert (o.validate_centerlines, o.centerline_max_iters, o.save_centerlines, o.save_best_metric) == (False, 64, False, "f1")
    o = parse_options(["--validate_centerlines", "--centerline_max_iters=100", "--save_best_metric=cl_quality", "--save_centerlines"])
    assert (o.validate_centerlines, o.centerline_max_iters, o.save_centerlines, o.save_best_metric) == (True, 100, True, "cl_quality")
    assert parse_options(["--novalidate_centerlines"]).validate_centerlines is False
    assert parse_options(["--validate_centerlines"]).validate_distances is False          # it does not need the distances flag
    assert M.parse_centerline_max_iters(1) == 1 and M.parse_centerline_max_iters("512") == 512
    assert isinstance(M.parse_centerline_max_iters(np.int64(3)), int) and M.parse_centerline_max_iters(4.0) == 4
    for bad in (0, -1, 513, 1.5, float("nan"), float("inf"), "x", "", None, True, 1 << 31, (1, 2)):
        with pytest.raises(ValueError, match="centerline_max_iters"):
            M.parse_centerline_max_iters(bad)
        with pytest.raises(ValueError):
            M.Options(centerline_max_iters=bad)
    assert M.parse_save_best_metric("cl_quality") == "cl_quality" and M.parse_save_best_metric("f1") == "f1"
    for bad in ("iou", "dice", "", "F1", "cldice_hard", "cl_completeness", None, 1, True):
        with pytest.raises(ValueError, match="save_best_metric"):
            M.parse_save_best_metric(bad)
        with pytest.raises(ValueError):
            M.Options(save_best_metric=bad, validate_centerlines=True)
    # cl_quality needs the centre-lines: refused when the options are checked, in the constructor and on the command line
    with pytest.raises(ValueError, match="validate_centerlines"):
        M.Options(save_best_metric="cl_quality")
    with pytest.raises(ValueError, match="validate_centerlines"):
        parse_options(["--save_best_metric=cl_quality", "--validate_distances"])
    with pytest.raises(ValueError, match="validate_distances"):
        parse_options(["--save_best_metric=relaxed_f1", "--validate_centerlines"])
    for bad in ("--centerline_max_iters=0", "--centerline_max_iters=513", "--save_best_metric=dice"):
        with pytest.raises(ValueError):
            parse_options(["--validate_centerlines", bad])
    with pytest.raises(SystemExit):
        parse_options(["--centerline_max_iters=some"])


# ------------------------------------------------------------------------------------------- thin_mask: the topology of its input
HOST_SHAPE = (2, 70, 83)
BIG_SHAPE = (1, 130, 133)


def _check_topology(mask, skel, what):
    assert skel.dtype == np.bool_ and skel.shape == mask.shape and not (skel & ~mask).any(), what
    for n in range(mask.shape[0]):
        assert TU.topology(skel[n]) == TU.topology(mask[n]), (what, n, TU.topology(skel[n]), TU.topology(mask[n]))


@pytest.mark.parametrize("kind", TU.KINDS)
def test_thin_mask_keeps_the_topology_and_is_idempotent(kind):
    for shape in (HOST_SHAPE, BIG_SHAPE) if kind.startswith("smooth") or kind == "ones" else (HOST_SHAPE,):
        mask = TU.masks(kind, shape)
        skel, deleted = hostio.thin_mask(mask, 512)
        assert deleted.dtype == np.int64 and deleted.shape == (shape[0],) and not deleted.any(), (kind, shape)
        _check_topology(mask, skel, (kind, shape))
        again, d2 = hostio.thin_mask(skel, 512)
        assert np.array_equal(again, skel) and not d2.any()
        for it in (1, 2, 3, 5):   # a truncated run keeps the topology too, and says whether it was cut short
            part, d = hostio.thin_mask(mask, it)
            _check_topology(mask, part, (kind, shape, it))
            assert not (skel & ~part).any()
            for n in range(shape[0]):   # nothing deleted by the last iteration: the image is at its fixed point
                assert d[n] != 0 or np.array_equal(part[n], skel[n])


def test_thin_mask_special_cases_and_argument_errors():
    lone = TU.masks("lone2x2", HOST_SHAPE)
    skel, _ = hostio.thin_mask(lone, 64)
    assert (skel.reshape(2, -1).sum(axis=1) == 1).all()                      # a lone 2 x 2 block thins to one pixel
    assert not hostio.thin_mask(TU.masks("zeros", HOST_SHAPE), 64)[0].any()
    ones, d = hostio.thin_mask(TU.masks("ones", BIG_SHAPE), 8)
    assert d[0] > 0 and ones.sum() < BIG_SHAPE[1] * BIG_SHAPE[2]              # eight iterations do not finish a 130 x 133 block
    full, d = hostio.thin_mask(TU.masks("ones", BIG_SHAPE), 512)
    assert d[0] == 0 and TU.topology(full[0]) == (1, 1)
    # a one-pixel line, a diagonal and a single pixel are their own skeletons
    m = np.zeros((3, 9, 9), bool)
    m[0, 4, 1:8] = True
    m[1][np.arange(1, 8), np.arange(1, 8)] = True
    m[2, 4, 4] = True
    assert np.array_equal(hostio.thin_mask(m, 64)[0], m)
    # images are independent: a stack gives what its images give alone
    stack = TU.masks("smooth3", HOST_SHAPE)
    both = hostio.thin_mask(stack, 64)[0]
    assert all(np.array_equal(hostio.thin_mask(stack[n:n + 1], 64)[0][0], both[n]) for n in range(2))
    for bad in (np.zeros((4, 4), bool), np.zeros((1, 4, 4), np.uint8), np.zeros((1, 0, 4), bool)):
        with pytest.raises(ValueError, match="thin_mask"):
            hostio.thin_mask(bad, 8)
    for bad in (0, 513, 1.5, True, None, "8"):
        with pytest.raises(ValueError, match="max_iters"):
            hostio.thin_mask(np.zeros((1, 4, 4), bool), bad)


def test_mask_thin_formats_and_counts():
    shape = (3, 63, 65)
    from tests import components_util as CU
    prob, labels = CU.float_bank(shape), TU.mixed_labels(shape)
    sp, st, counts, info = hostio.mask_thin(prob, 0.5, labels, 64)
    counted = (labels == 0) | (labels == 1)
    with np.errstate(invalid="ignore"):
        P, T = (prob >= np.float32(0.5)) & counted, labels == 1
    assert sp.dtype == np.float32 and st.dtype == np.int64 and counts.dtype == np.int64 and info.dtype == np.uint32 and info.shape == (3, 2)
    assert set(np.unique(sp)) <= {0.0, 1.0} and np.array_equal(sp > 0, hostio.thin_mask(P, 64)[0])
    assert np.array_equal(st[~counted], labels[~counted]) and np.array_equal(st[counted] == 1, hostio.thin_mask(T, 64)[0][counted])
    S_P, S_T = sp > 0, (st == 1) & counted
    assert list(counts) == [S_P.sum(), (S_P & T).sum(), S_T.sum(), (S_T & P).sum()] and counts[1] <= counts[0] and counts[3] <= counts[2]
    assert not S_P[-1].any() and (st[-1] == -1).all() and not info.any()      # the all-ignored image
    # the outputs are what rsu_distance_hist reads: the skeletons come back as its two masks
    h = hostio.distance_hist(sp, 0.5, st)
    assert h[0].sum() == counts[0] and h[1].sum() == counts[2]
    cut = hostio.mask_thin(prob, 0.5, (T & counted).astype(np.int64) * 0 + TU.masks("smooth6", shape), 1)[3]
    assert cut[:, 1].all()                                                    # one iteration does not finish a smooth blob
    free = hostio.mask_thin(prob, 0.5, None, 64)
    assert free[1] is None and free[2][1] == 0 and free[2][2] == 0 and not free[3][:, 1].any()
    with pytest.raises(ValueError):
        hostio.mask_thin(prob, float("nan"), labels, 64)
    with pytest.raises(ValueError):
        hostio.mask_thin(prob, 0.5, labels[:2], 64)
    with pytest.raises(ValueError, match="max_iters"):
        hostio.mask_thin(prob, 0.5, labels, 0)


# ------------------------------------------------------------------------------------------- centerline_metrics
def test_centerline_metrics_hand_counted():
    h = np.zeros((2, 64), np.int64)
    h[0, :4] = (6, 2, 1, 1)      # ten predicted skeleton pixels: 6 on the true centre-line, 2 one pixel off, ...
    h[0, 63] = 10                # ... and ten with no true centre-line within 62 pixels
    h[1, :3] = (6, 3, 1)
    h[1, 10] = 6
    counts = np.array([20, 15, 16, 4], np.int64)
    m = hostio.centerline_metrics(h, counts, 1)
    corr, comp = 8 / 20, 9 / 16
    assert m["cl_correctness"] == corr and m["cl_completeness"] == comp
    assert m["cl_quality"] == comp * corr / (comp - comp * corr + corr)
    tprec, tsens = 15 / 20, 4 / 16
    assert m["cldice_hard"] == 2 * tprec * tsens / (tprec + tsens) and (m["cl_len_pred"], m["cl_len_true"]) == (20, 16)
    assert set(m) == {"cl_correctness", "cl_completeness", "cl_quality", "cldice_hard", "cl_len_pred", "cl_len_true"}
    m0 = hostio.centerline_metrics(h, counts, 0)
    assert (m0["cl_correctness"], m0["cl_completeness"]) == (6 / 20, 6 / 16)
    assert hostio.centerline_metrics(h, counts, 62)["cl_correctness"] == 0.5 and hostio.centerline_metrics(h, counts, 62)["cl_completeness"] == 1.0
    # quality = TP / (TP + FP + FN) when both sides count the same matches: 1 for identical centre-lines
    same = np.zeros((2, 64), np.int64)
    same[:, 0] = 7
    assert hostio.centerline_metrics(same, [7, 7, 7, 7], 0) == {"cl_correctness": 1.0, "cl_completeness": 1.0, "cl_quality": 1.0,
                                                                   "cldice_hard": 1.0, "cl_len_pred": 7, "cl_len_true": 7}
    # empty sides: denominators max(., 1), no division by zero, everything 0
    empty = hostio.centerline_metrics(np.zeros((2, 64), np.int64), np.zeros(4, np.int64), 3)
    assert empty == {"cl_correctness": 0.0, "cl_completeness": 0.0, "cl_quality": 0.0, "cldice_hard": 0.0, "cl_len_pred": 0, "cl_len_true": 0}
    one = np.zeros((2, 64), np.int64)
    one[0, 63] = 5               # a prediction without any truth
    m1 = hostio.centerline_metrics(one, [5, 0, 0, 0], 3)
    assert (m1["cl_correctness"], m1["cl_completeness"], m1["cl_quality"], m1["cldice_hard"]) == (0.0, 0.0, 0.0, 0.0)
    assert "proxy" in hostio.centerline_metrics.__doc__
    for bad in (np.zeros((2, 63), np.int64), np.zeros((2, 64), np.float64), np.zeros(128, np.int64)):
        with pytest.raises(ValueError, match="cl_hist"):
            hostio.centerline_metrics(bad, counts, 1)
    for bad in (np.zeros(3, np.int64), np.zeros(4, np.float64), np.array([1, -1, 1, 1]), 5):
        with pytest.raises(ValueError, match="counts"):
            hostio.centerline_metrics(h, bad, 1)
    for bad in (-1, 63, 1.0, True, None, "1"):
        with pytest.raises(ValueError, match="slack"):
            hostio.centerline_metrics(h, counts, bad)
