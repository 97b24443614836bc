"""No GPU: the seventh public header include/rsu_distance.h (mask distances). The library exports what the header declares and
_lib.SIGNATURES_DISTANCE binds exactly that, disjoint from the other six tables, which did not grow; the size function and every
refusal with NULL device pointers; the 2-GiB refusal one image past the limit; tests/test_gpu_distance_fenced.py leaves no launching
entry of the header out; the flags, their parsers and refusals; the host restatements of hostio against scipy's distance transform and
against a brute-force minimum; the bin rule; the histogram's properties and relaxed_metrics."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from road_segmentation_unet_amd import _lib, hostio
from road_segmentation_unet_amd import model as M
from road_segmentation_unet_amd.cli import parse_options
from tests import components_util as CU
from tests import distance_util as DU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
ENTRIES = ["rsu_distance_hist", "rsu_distance_ws_bytes", "rsu_mask_distance"]
LAUNCHING = ["rsu_distance_hist", "rsu_mask_distance"]
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
def test_library_exports_the_seventh_header_and_the_table_binds_it():
    L = _lib.lib()
    syms = _symbols("rsu_distance.h")
    assert syms == ENTRIES
    for s in syms:
        assert hasattr(L, s), "librsu_hip.so does not export %s" % s
        assert getattr(L, s).argtypes == _lib.SIGNATURES_DISTANCE[s][1] and getattr(L, s).restype is _lib.SIGNATURES_DISTANCE[s][0]
    assert sorted(_lib.SIGNATURES_DISTANCE) == syms, "ctypes table and rsu_distance.h out of sync"
    tables = [set(_lib.SIGNATURES), set(_lib.SIGNATURES_OPTIM), set(_lib.SIGNATURES_LOSS), set(_lib.SIGNATURES_CLDICE),
              set(_lib.SIGNATURES_LOVASZ), set(_lib.SIGNATURES_COMPONENTS), set(_lib.SIGNATURES_DISTANCE)]
    for i in range(7):
        for j in range(i + 1, 7):
            assert not (tables[i] & tables[j]), (i, j)
    # the other six headers declare what they did: the new entries live in the seventh
    assert sorted(_lib.SIGNATURES) == _symbols("rsu.h") and len(_lib.SIGNATURES) == N_RSU_H
    assert sorted(_lib.SIGNATURES_OPTIM) == _symbols("rsu_optim.h") == ["rsu_update_table_run_adam_decay", "rsu_update_table_run_decay"]
    assert sorted(_lib.SIGNATURES_LOSS) == _symbols("rsu_loss.h") == ["rsu_head_eval_focal", "rsu_head_fwd_bwd_focal"]
    assert sorted(_lib.SIGNATURES_CLDICE) == _symbols("rsu_cldice.h") == ["rsu_cldice_bwd", "rsu_cldice_fwd", "rsu_cldice_ws_floats", "rsu_head_fwd_bwd_aux"]
    assert sorted(_lib.SIGNATURES_LOVASZ) == _symbols("rsu_lovasz.h") == ["rsu_lovasz_fwd", "rsu_lovasz_fwd_bwd", "rsu_lovasz_ws_bytes"]
    assert sorted(_lib.SIGNATURES_COMPONENTS) == _symbols("rsu_components.h") == ["rsu_components_filter", "rsu_components_label",
                                                                                "rsu_components_pair_count", "rsu_components_ws_bytes"]
    others = ("rsu.h", "rsu_optim.h", "rsu_loss.h", "rsu_cldice.h", "rsu_lovasz.h", "rsu_components.h")
    assert not [n for h in others for n in _symbols(h) if "distance" in n]
    assert '#include "rsu.h"' in _header("rsu_distance.h")
    for macro, value in (("RSU_DIST_BINS", "64"), ("RSU_DIST_NONE", "0x7fffffff"), ("RSU_DIST_MAX_SIDE", "1024")):
        assert re.search(r"^#define %s %s$" % (macro, value), _header("rsu_distance.h"), flags=re.M), macro
    assert (_lib.DIST_BINS, _lib.DIST_NONE, _lib.DIST_MAX_SIDE) == (64, 0x7fffffff, 1024) == (hostio.DIST_BINS, hostio.DIST_NONE, hostio.DIST_MAX_SIDE)
    # the argument lists of the header and of the table: the same lengths, floats (by value) and ints in the same positions
    protos = _protos("rsu_distance.h")
    assert sorted(n for _, n, _ in protos) == ENTRIES
    for ret, name, args in protos:
        kinds = []
        for a in args.split(","):
            a = " ".join(a.split())
            kinds.append("f" if re.fullmatch(r"float \w+", a) else "l" if re.fullmatch(r"long \w+", a) else "i" if re.fullmatch(r"int \w+", a) else "p")
            assert kinds[-1] != "p" or "*" in a or a.startswith("rsu_stream_t "), (name, a)
        table = ["f" if t is _lib._f else "l" if t is _lib._l else "i" if t is _lib._i else "p" for t in _lib.SIGNATURES_DISTANCE[name][1]]
        assert kinds == table, (name, kinds, table)
        assert _lib.SIGNATURES_DISTANCE[name][0] is (_lib._sz if ret == "size_t" else _lib._i)


N_RSU_H = 94   # the entries of include/rsu.h before this header came: the first table did not grow


def test_size_function_and_refusals_without_a_gpu():
    L = _lib.lib()
    for shape in DU.SHAPES + [(4, 388, 388), (2, 608, 608), (1, 1024, 1024), (255, 1024, 1024), (511, 1024, 1024)]:
        assert L.rsu_distance_ws_bytes(*shape) == 4 * shape[0] * shape[1] * shape[2], shape
    assert "4 * N * H * W" in " ".join(open(os.path.join(ROOT, "include", "rsu_distance.h")).read().split())
    bad_sizes = ((0, 5, 5), (5, 0, 5), (5, 5, 0), (-1, 5, 5), (5, -1, 5), (5, 5, -1), (1, 1025, 5), (1, 5, 1025), (1, 1 << 20, 1))
    for bad in bad_sizes + ((512, 1024, 1024), (1 << 30, 2, 1)):
        assert L.rsu_distance_ws_bytes(*bad) == 0, bad
    # refused before anything is launched or dereferenced: NULL pointers, and pointers nobody may follow
    ok = (2, 5, 7)
    assert L.rsu_mask_distance(None, 0.5, None, None, None, None, *ok, None) == EINVAL
    assert L.rsu_distance_hist(None, 0.5, None, None, None, *ok, None) == EINVAL
    assert L.rsu_mask_distance(None, 0.5, p, p, p, p, *ok, None) == EINVAL       # prob
    assert L.rsu_mask_distance(p, 0.5, p, p, p, None, *ok, None) == EINVAL       # ws
    assert L.rsu_mask_distance(p, 0.5, p, None, None, p, *ok, None) == EINVAL    # both outputs
    assert L.rsu_mask_distance(p, 0.5, None, p, p, p, *ok, None) == EINVAL       # d2_true without labels
    assert L.rsu_mask_distance(p, 0.5, None, None, p, p, *ok, None) == EINVAL
    for i in range(5):                                                           # prob, labels64, acc, ws of the histogram
        args = [p, 0.5, p, p, p]
        if i != 1:
            args[i] = None
            assert L.rsu_distance_hist(*args, *ok, None) == EINVAL, i
    for bad in bad_sizes:
        assert L.rsu_mask_distance(p, 0.5, p, p, p, p, *bad, None) == EINVAL, bad
        assert L.rsu_distance_hist(p, 0.5, p, p, p, *bad, None) == EINVAL, bad
    for t in (float("nan"), float("inf"), float("-inf")):
        assert L.rsu_mask_distance(p, t, p, p, p, p, *ok, None) == EINVAL
        assert L.rsu_distance_hist(p, t, p, p, p, *ok, None) == EINVAL


def test_two_gib_refusal_one_image_past_the_limit():
    """at 1024 x 1024 labels64 takes 8 MiB per image: 255 images are the last batch below 0x7ffffff0 bytes, 256 reach 2 GiB. Without
    labels64 the largest tensor has 4 bytes per pixel: 511 images pass, 512 do not."""
    L = _lib.lib()
    S = 1024
    assert 255 * S * S * 8 < 0x7ffffff0 <= 256 * S * S * 8 and 511 * S * S * 4 < 0x7ffffff0 <= 512 * S * S * 4
    assert L.rsu_distance_ws_bytes(255, S, S) == 255 * S * S * 4
    assert L.rsu_distance_hist(p, 0.5, p, p, p, 256, S, S, None) == _lib.E2BIG
    assert L.rsu_mask_distance(p, 0.5, p, p, p, p, 256, S, S, None) == _lib.E2BIG
    assert L.rsu_mask_distance(p, 0.5, p, p, None, p, 256, S, S, None) == _lib.E2BIG    # labels64 given: it is the largest tensor
    assert L.rsu_mask_distance(p, 0.5, None, p, None, p, 512, S, S, None) == _lib.E2BIG
    with pytest.raises(_lib.RsuError, match="2 GiB"):
        _lib.call("rsu_distance_hist", p, 0.5, p, p, p, 256, S, S, None)
    # a wrong argument is reported before the size
    assert L.rsu_distance_hist(p, float("nan"), p, p, p, 256, S, S, None) == EINVAL
    assert L.rsu_distance_hist(None, 0.5, p, p, p, 256, S, S, None) == EINVAL


def test_the_fenced_file_covers_every_launching_entry_of_the_seventh_header():
    """tests/test_components_host.py's rule for rsu_components.h, for rsu_distance.h and tests/test_gpu_distance_fenced.py"""
    from tests import test_gpu_distance_fenced as G
    protos = _protos("rsu_distance.h")
    launching = [n for r, n, a in protos if r == "int" and "rsu_stream_t" in a]
    assert sorted(launching) == LAUNCHING and [n for r, n, a in protos if r == "size_t"] == ["rsu_distance_ws_bytes"]
    tests = {n: f for n, f in vars(G).items() if n.startswith("test_") and callable(f)}
    assert sorted(G.FENCED) == LAUNCHING
    for entry, names in G.FENCED.items():
        assert names, entry
        for n in names:
            assert n in tests, (entry, n)
            assert re.search(r'"%s"' % entry, inspect.getsource(tests[n]) + "".join(inspect.getsource(h) for h in G.HELPERS.get(n, ()))), \
                "%s is not launched by %s" % (entry, n)
    assert "pytest.mark.gpu" in inspect.getsource(G)
    assert "rsu_distance_ws_bytes" in inspect.getsource(G)   # exact workspaces


# ------------------------------------------------------------------------------------------- the flags and their parsers
def test_flags_defaults_parsers_and_refusals():
    defs = {d[0]: d for d in M.EXTRA_FLAG_DEFS}
    assert defs["validate_distances"][1:3] == (bool, False) and defs["relaxed_slack"][1:3] == (int, 3)
    assert defs["save_best_metric"][1:3] == (str, "f1")
    for o in (M.Options(), parse_options([])):
        assert (o.validate_distances, o.relaxed_slack, o.save_best_metric) == (False, 3, "f1")
    o = parse_options(["--validate_distances", "--relaxed_slack=5", "--save_best_metric=relaxed_f1"])
    assert (o.validate_distances, o.relaxed_slack, o.save_best_metric) == (True, 5, "relaxed_f1")
    assert parse_options(["--novalidate_distances"]).validate_distances is False
    assert parse_options(["--validate_distances", "--save_best_metric=f1"]).save_best_metric == "f1"
    assert M.parse_relaxed_slack(0) == 0 and M.parse_relaxed_slack("62") == 62 and isinstance(M.parse_relaxed_slack(np.int64(3)), int)
    assert M.parse_relaxed_slack(4.0) == 4
    for bad in (-1, 63, 1.5, float("nan"), float("inf"), "x", "", None, True, 1 << 31, (1, 2)):
        with pytest.raises(ValueError, match="relaxed_slack"):
            M.parse_relaxed_slack(bad)
        with pytest.raises(ValueError):
            M.Options(relaxed_slack=bad)
    assert M.parse_save_best_metric("f1") == "f1" and M.parse_save_best_metric("relaxed_f1") == "relaxed_f1"
    for bad in ("iou", "", "F1", None, 1, True):
        with pytest.raises(ValueError, match="save_best_metric"):
            M.parse_save_best_metric(bad)
        with pytest.raises(ValueError):
            M.Options(save_best_metric=bad, validate_distances=True)
    # relaxed_f1 needs the distances: refused when the options are checked, in the constructor and on the command line
    with pytest.raises(ValueError, match="validate_distances"):
        M.Options(save_best_metric="relaxed_f1")
    with pytest.raises(ValueError, match="validate_distances"):
        parse_options(["--save_best_metric=relaxed_f1"])
    for bad in ("--relaxed_slack=-1", "--relaxed_slack=63", "--save_best_metric=dice"):
        with pytest.raises(ValueError):
            parse_options(["--validate_distances", bad])
    with pytest.raises(SystemExit):
        parse_options(["--relaxed_slack=some"])
    assert "outside the patch" in " ".join(defs["validate_distances"][3].split())


# ------------------------------------------------------------------------------------------- hostio against scipy and brute force
HOST_SHAPES = DU.SHAPES + [DU.ALL_BINS_SHAPE]


@pytest.mark.parametrize("shape", HOST_SHAPES, ids=[DU.shape_id(s) for s in HOST_SHAPES])
def test_mask_distance_against_scipy(shape):
    for name in DU.pair_names(shape):
        prob, labels = DU.pair(name, shape)
        d2p, d2t, _ = DU.host_pair(name, shape)
        assert d2p.dtype == np.int32 and d2t.dtype == np.int32 and d2p.shape == shape and d2t.shape == shape
        P, T = DU.masks_of(prob, labels)
        for n in range(shape[0]):
            assert np.array_equal(d2p[n], DU.scipy_d2(P[n])), (name, shape, n, "pred")
            assert np.array_equal(d2t[n], DU.scipy_d2(T[n])), (name, shape, n, "true")
        assert np.array_equal(d2p == 0, P) and np.array_equal(d2t == 0, T)
    if shape[0] > 1:   # images do not see each other
        d2p, d2t, hist = DU.host_pair("neighbours", shape)
        assert (d2p[1] == DU.NONE).all() and (d2t[0] == DU.NONE).all() and hist[0, -1] == 1 and hist[1, -1] == 1 and hist.sum() == 2


@pytest.mark.parametrize("shape", [(1, 1, 1), (2, 1, 70), (2, 70, 1), (3, 63, 65), (1, 40, 90)], ids=DU.shape_id)
def test_mask_distance_and_scipy_against_brute_force(shape):
    for name in ("rand0.41~shift", "spiral~rings", "checker~shift", "rand0.41~empty", "empty~rand0.41"):
        prob, labels = DU.pair(name, shape)
        d2p, d2t = hostio.mask_distance(prob, DU.THRESHOLD, labels)
        P, T = DU.masks_of(prob, labels)
        for n in range(shape[0]):
            assert np.array_equal(d2p[n], DU.brute_d2(P[n])) and np.array_equal(d2t[n], DU.brute_d2(T[n])), (name, shape, n)
            assert np.array_equal(DU.scipy_d2(P[n]), DU.brute_d2(P[n])), (name, shape, n)


def test_single_far_pixels_and_special_values():
    # one mask pixel at a corner of 150 x 150: d2 up to 2 * 149^2 = 44402, every value a sum of two squares
    prob = np.zeros((1, 150, 150), f32)
    prob[0, -1, -1] = 1
    d2p, d2t = hostio.mask_distance(prob, 0.5)
    yy, xx = np.mgrid[0:150, 0:150]
    assert np.array_equal(d2p[0], (149 - yy) ** 2 + (149 - xx) ** 2) and d2p.max() == 44402 and (d2t == DU.NONE).all()
    # the threshold itself, the float below it, -0.0, NaN, infinities; labels beside them: -1, 2 and (1 << 32) | 1 are not counted
    pr = np.array([[[0.5, np.nextafter(f32(0.5), f32(0)), -0.0, np.nan, np.inf, -np.inf, 0.75, 0.9, 0.9, 0.9]]], f32)
    lab = np.array([[[0, 0, 1, 1, 0, 0, 1, -1, 2, (1 << 32) | 1]]], np.int64)
    P, T = DU.masks_of(pr, lab)
    assert P[0, 0].tolist() == [True, False, False, False, True, False, True, False, False, False]
    assert T[0, 0].tolist() == [False, False, True, True, False, False, True, False, False, False]
    d2p, d2t = hostio.mask_distance(pr, 0.5, lab)
    assert d2p[0, 0].tolist() == [0, 1, 4, 1, 0, 1, 0, 1, 4, 9] and d2t[0, 0].tolist() == [4, 1, 0, 0, 1, 1, 0, 1, 4, 9]
    hist = hostio.distance_hist(pr, 0.5, lab)
    assert hist[0].tolist() == [1, 1, 1] + [0] * 61 and hist[1].tolist() == [1, 1, 1] + [0] * 61
    assert np.array_equal(hostio.mask_distance(pr, 0.5)[0][0, 0], [0, 1, 2 * 2, 1, 0, 1, 0, 0, 0, 0])   # without labels every pixel is counted
    for bad in (np.nan, np.inf):
        with pytest.raises(ValueError):
            hostio.mask_distance(pr, bad)
    with pytest.raises(ValueError):
        hostio.mask_distance(pr[0], 0.5)
    with pytest.raises(ValueError):
        hostio.mask_distance(np.zeros((1, 1025, 2), f32), 0.5)
    with pytest.raises(ValueError):
        hostio.distance_hist(pr, 0.5, None)
    with pytest.raises(ValueError):
        hostio.distance_hist(pr, 0.5, lab[:, :, :5])


def test_the_bin_rule_at_the_squares_and_just_past_them():
    r = np.arange(70, dtype=np.int64)
    assert np.array_equal(hostio.distance_bin(r * r), np.minimum(r, 63))
    assert np.array_equal(hostio.distance_bin(r * r + 1), np.minimum(r + 1, 63))
    assert hostio.distance_bin(DU.NONE) == 63 and hostio.distance_bin(0) == 0 and hostio.distance_bin(62 * 62) == 62
    d2 = np.arange(0, 5000, dtype=np.int64)
    for rho in (0, 1, 3, 17, 62):   # d2 <= rho^2 iff bin <= rho
        assert np.array_equal(d2 <= rho * rho, hostio.distance_bin(d2) <= rho), rho


@pytest.mark.parametrize("shape", [(3, 63, 65), (2, 130, 67), DU.ALL_BINS_SHAPE], ids=DU.shape_id)
def test_distance_hist_properties_and_relaxed_metrics(shape):
    labels_mixed = DU.mixed_labels(shape)
    cases = [(n,) + DU.pair(n, shape) for n in DU.pair_names(shape)] + [("float_bank", CU.float_bank(shape), labels_mixed)]
    for name, prob, labels in cases:
        hist = hostio.distance_hist(prob, DU.THRESHOLD, labels)
        assert hist.dtype == np.int64 and hist.shape == (2, 64)
        P, T = DU.masks_of(prob, labels)
        assert hist[0].sum() == P.sum() and hist[1].sum() == T.sum() and hist[0, 0] == hist[1, 0] == (P & T).sum(), name
        m = hostio.relaxed_metrics(hist, 0)   # at slack 0: the confusion counts' precision and recall
        tp, fp, fn = float((P & T).sum()), float((P & ~T).sum()), float((T & ~P).sum())
        assert m["relaxed_precision"] == tp / max(tp + fp, 1.0) and m["relaxed_recall"] == tp / max(tp + fn, 1.0), name
        for rho in (1, 3, 62):
            r = hostio.relaxed_metrics(hist, rho)
            assert r["relaxed_precision"] == hist[0, :rho + 1].sum() / max(hist[0].sum(), 1)
            assert r["relaxed_recall"] == hist[1, :rho + 1].sum() / max(hist[1].sum(), 1)
            pr, rc = r["relaxed_precision"], r["relaxed_recall"]
            assert r["relaxed_f1"] == (2.0 * pr * rc / (pr + rc) if pr + rc > 0 else 0.0)
            assert r["relaxed_precision"] >= m["relaxed_precision"] and r["relaxed_recall"] >= m["relaxed_recall"]
        assert r["far_pred"] == hist[0, 63] / max(hist[0].sum(), 1) and r["far_true"] == hist[1, 63] / max(hist[1].sum(), 1)
        assert r["mean_dist_pred"] == float((hist[0] * np.arange(64)).sum()) / max(hist[0].sum(), 1)
        if shape[0] > 1 and name == "float_bank":   # the last image is ignored altogether: it adds exactly nothing
            assert np.array_equal(hist, hostio.distance_hist(prob[:-1], DU.THRESHOLD, labels[:-1]))
    if shape == DU.ALL_BINS_SHAPE:   # every bin of hist[0], the saturated one included
        hist = DU.host_pair("full~corner", shape)[2]
        assert (hist[0] > 0).all() and hist[0, 63] == 32844 and hist[0].sum() == 39000 and hist[1].tolist() == [2] + [0] * 63
    none = hostio.distance_hist(CU.float_bank(shape), DU.THRESHOLD, np.full(shape, -1, np.int64))
    assert not none.any()
    z = hostio.relaxed_metrics(none, 3)
    assert set(z) == {"relaxed_precision", "relaxed_recall", "relaxed_f1", "mean_dist_pred", "mean_dist_true", "far_pred", "far_true"}
    assert not any(z.values())
    assert "SATURATING" in hostio.relaxed_metrics.__doc__
    for bad in (-1, 63, 1.5, None, True):
        with pytest.raises(ValueError):
            hostio.relaxed_metrics(none, bad)
    with pytest.raises(ValueError):
        hostio.relaxed_metrics(none[:, :10], 3)


def test_hostio_distance_needs_neither_torch_nor_scipy():
    for fn in (hostio.mask_distance, hostio.distance_hist, hostio.relaxed_metrics, hostio.distance_bin, hostio._dist_transform):
        assert "scipy" not in inspect.getsource(fn) and "torch" not in inspect.getsource(fn), fn.__name__
