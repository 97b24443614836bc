"""No GPU: the sixth public header include/rsu_components.h (connected components). The library exports what the header declares and
_lib.SIGNATURES_COMPONENTS binds exactly that, disjoint from the other five tables, which did not grow; the size function and the
refusals; tests/test_gpu_components_fenced.py leaves no launching entry of the header out (the rule of tests/test_lovasz_host.py); the
flags, their parsers and refusals; the host restatements of hostio against scipy.ndimage over the bank of tests/components_util.py; the
serial restatement of the kernels' own steps (tiles, hierarchical border merges, flatten) against the same; postprocess_masks as the
identity."""
import inspect
import os
import re

import numpy as np
import pytest

from road_segmentation_unet_amd import _lib, hostio
from road_segmentation_unet_amd import model as M
from road_segmentation_unet_amd.cli import parse_options
from tests import components_util as CU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
f32 = np.float32
ENTRIES = ["rsu_components_filter", "rsu_components_label", "rsu_components_pair_count", "rsu_components_ws_bytes"]
LAUNCHING = ["rsu_components_filter", "rsu_components_label", "rsu_components_pair_count"]
SHAPE_IDS = [CU.shape_id(s) for s in CU.SHAPES]


def _header(name):
    txt = open(os.path.join(ROOT, "include", name)).read()
    return re.sub(r"/\*.*?\*/", " ", txt, flags=re.S)


def _symbols(name):
    return sorted(set(re.findall(r"\b(rsu_[a-zA-Z0-9_]+)\s*\(", _header(name))))


def _protos(name):
    return re.findall(r"^(int|size_t) (rsu_\w+)\(([^;]*?)\);", _header(name), flags=re.M | re.S)


# ------------------------------------------------------------------------------------------- ABI
def test_library_exports_the_sixth_header_and_the_table_binds_it():
    L = _lib.lib()
    syms = _symbols("rsu_components.h")
    assert syms == ENTRIES
    for s in syms:
        assert hasattr(L, s), "librsu_hip.so does not export %s" % s
        assert getattr(L, s).argtypes == _lib.SIGNATURES_COMPONENTS[s][1] and getattr(L, s).restype is _lib.SIGNATURES_COMPONENTS[s][0]
    assert sorted(_lib.SIGNATURES_COMPONENTS) == syms, "ctypes table and rsu_components.h out of sync"
    tables = [set(_lib.SIGNATURES), set(_lib.SIGNATURES_OPTIM), set(_lib.SIGNATURES_LOSS), set(_lib.SIGNATURES_CLDICE),
              set(_lib.SIGNATURES_LOVASZ), set(_lib.SIGNATURES_COMPONENTS)]
    for i in range(6):
        for j in range(i + 1, 6):
            assert not (tables[i] & tables[j]), (i, j)
    # the other five headers declare what they did: the new entries live in the sixth
    assert sorted(_lib.SIGNATURES) == _symbols("rsu.h") and sorted(_lib.SIGNATURES_OPTIM) == _symbols("rsu_optim.h")
    assert sorted(_lib.SIGNATURES_LOSS) == _symbols("rsu_loss.h") == ["rsu_head_eval_focal", "rsu_head_fwd_bwd_focal"]
    assert sorted(_lib.SIGNATURES_CLDICE) == _symbols("rsu_cldice.h") == ["rsu_cldice_bwd", "rsu_cldice_fwd", "rsu_cldice_ws_floats", "rsu_head_fwd_bwd_aux"]
    assert sorted(_lib.SIGNATURES_LOVASZ) == _symbols("rsu_lovasz.h") == ["rsu_lovasz_fwd", "rsu_lovasz_fwd_bwd", "rsu_lovasz_ws_bytes"]
    assert not [n for h in ("rsu.h", "rsu_optim.h", "rsu_loss.h", "rsu_cldice.h", "rsu_lovasz.h") for n in _symbols(h) if "components" in n]
    assert '#include "rsu.h"' in _header("rsu_components.h")
    # the argument lists of the header and of the table: the same lengths, floats (by value) and ints in the same positions
    protos = _protos("rsu_components.h")
    assert sorted(n for _, n, _ in protos) == ENTRIES
    for ret, name, args in protos:
        kinds = []
        for a in args.split(","):
            a = " ".join(a.split())
            kinds.append("f" if re.fullmatch(r"float \w+", a) else "l" if re.fullmatch(r"long \w+", a) else "i" if re.fullmatch(r"int \w+", a) else "p")
            assert kinds[-1] != "p" or "*" in a or a.startswith("rsu_stream_t "), (name, a)
        table = ["f" if t is _lib._f else "l" if t is _lib._l else "i" if t is _lib._i else "p" for t in _lib.SIGNATURES_COMPONENTS[name][1]]
        assert kinds == table, (name, kinds, table)
        assert _lib.SIGNATURES_COMPONENTS[name][0] is (_lib._sz if ret == "size_t" else _lib._i)


def _ws_formula(N, H, W):
    """rsu_components.h: five int32 arrays of N * H * W elements and four int32 counters per image"""
    return 5 * 4 * N * H * W + 4 * 4 * N


def test_size_function_and_refusals_without_a_gpu():
    L = _lib.lib()
    for shape in CU.SHAPES + [(4, 388, 388), (2, 608, 608), (1, 4096, 4096), (127, 4096, 4096), (1, 1, 1 << 24), (1, 1 << 24, 1)]:
        assert L.rsu_components_ws_bytes(*shape) == _ws_formula(*shape), shape
    assert "20 * N * H * W + 16 * N" in " ".join(open(os.path.join(ROOT, "include", "rsu_components.h")).read().split())
    for bad in ((0, 5, 5), (5, 0, 5), (5, 5, 0), (-1, 5, 5), (1, 4096, 4097), (1, 1 << 13, 1 << 12), (128, 4096, 4096), (1 << 30, 2, 1)):
        assert L.rsu_components_ws_bytes(*bad) == 0, bad
    # refused before anything is launched: NULL pointers never reach a device
    assert L.rsu_components_label(None, 0.5, 8, 0, None, None, None, None, 1, 5, 5, None) == -22
    assert L.rsu_components_filter(None, 0.5, 8, 2, 2, None, None, None, 1, 5, 5, None) == -22
    assert L.rsu_components_pair_count(None, 0.5, None, 8, None, None, 1, 5, 5, None) == -22


def test_the_fenced_file_covers_every_launching_entry_of_the_sixth_header():
    """tests/test_lovasz_host.py's rule for rsu_lovasz.h, for rsu_components.h and tests/test_gpu_components_fenced.py"""
    from tests import test_gpu_components_fenced as G
    protos = _protos("rsu_components.h")
    launching = [n for r, n, a in protos if r == "int" and "rsu_stream_t" in a]
    assert sorted(launching) == LAUNCHING and [n for r, n, a in protos if r == "size_t"] == ["rsu_components_ws_bytes"]
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
    assert "rsu_components_ws_bytes" in inspect.getsource(G)   # exact workspaces


# ------------------------------------------------------------------------------------------- the flags and their parsers
def test_flags_defaults_parsers_and_refusals():
    defs = {d[0]: d for d in M.EXTRA_FLAG_DEFS}
    assert defs["min_road_area"][1:3] == (int, 0) and defs["max_hole_area"][1:3] == (int, 0)
    assert defs["component_connectivity"][1:3] == (int, 8) and defs["validate_components"][1:3] == (bool, False)
    for o in (M.Options(), parse_options([])):
        assert (o.min_road_area, o.max_hole_area, o.component_connectivity, o.validate_components) == (0, 0, 8, False)
    o = parse_options(["--min_road_area=30", "--max_hole_area=12", "--component_connectivity=4", "--validate_components"])
    assert (o.min_road_area, o.max_hole_area, o.component_connectivity, o.validate_components) == (30, 12, 4, True)
    assert parse_options(["--novalidate_components"]).validate_components is False
    assert M.parse_component_area(0) == 0 and M.parse_component_area("17") == 17 and isinstance(M.parse_component_area(np.int64(3)), int)
    assert M.parse_component_area(5.0, "max_hole_area") == 5
    for bad in (-1, 1.5, float("nan"), float("inf"), "x", "", None, True, 1 << 31, (1, 2)):
        for name in ("min_road_area", "max_hole_area"):
            with pytest.raises(ValueError, match=name):
                M.parse_component_area(bad, name)
            with pytest.raises(ValueError):
                M.Options(**{name: bad})
    assert M.parse_component_connectivity(4) == 4 and M.parse_component_connectivity("8") == 8
    for bad in (0, 6, -4, 4.5, "four", None, True, float("nan")):
        with pytest.raises(ValueError):
            M.parse_component_connectivity(bad)
        with pytest.raises(ValueError):
            M.Options(component_connectivity=bad)
    for bad in ("--min_road_area=-1", "--max_hole_area=-3", "--component_connectivity=6"):
        with pytest.raises(ValueError):
            parse_options([bad])
    with pytest.raises(SystemExit):
        parse_options(["--min_road_area=some"])
    text = " ".join(defs["component_connectivity"][3].split())
    assert "dual" in text and "0 = off" in defs["min_road_area"][3] and "0 = off" in defs["max_hole_area"][3]


def test_postprocess_masks_is_the_identity_without_a_launch(monkeypatch):
    from road_segmentation_unet_amd import mask_metrics      # (it issues the tool's calls and asks the library for its workspace)
    calls = []
    for mod in (M, mask_metrics):
        monkeypatch.setattr(mod, "call", lambda *a: calls.append(a))
    monkeypatch.setattr(mask_metrics, "lib", lambda: calls.append("lib"))
    m = object.__new__(M.ConvolutionalModel)
    m._options = M.Options()
    masks = np.random.RandomState(0).rand(2, 9, 7, 1)
    assert m.postprocess_masks(masks) is masks and m.postprocess_masks(masks, threshold=0.25) is masks
    assert calls == [] and m.last_postprocess_stats is None
    assert inspect.signature(M.ConvolutionalModel.postprocess_masks).parameters["threshold"].default == 0.5
    m._options = M.Options(min_road_area=2)
    with pytest.raises(ValueError):
        m.postprocess_masks(masks[..., 0])


# ------------------------------------------------------------------------------------------- hostio against scipy
@pytest.mark.parametrize("connectivity", CU.CONNECTIVITIES)
@pytest.mark.parametrize("shape", CU.SHAPES + [(1, 131, 67)], ids=SHAPE_IDS + ["1x131x67"])
def test_label_components_against_scipy(shape, connectivity):
    for kind in CU.KINDS:
        mask = CU.masks(kind, shape)
        for invert in (False, True):
            labels, area, edge = CU.host_labels(kind, shape, connectivity, invert)
            assert labels.dtype == np.int32 and area.dtype == np.int32 and edge.dtype == np.uint8 and labels.shape == shape
            for n in range(shape[0]):
                fg = ~mask[n] if invert else mask[n]
                want = CU.scipy_labels(fg, connectivity)
                what = (kind, shape, connectivity, invert, n)
                assert np.array_equal(labels[n], want), what
                counts = np.bincount(want.reshape(-1), minlength=2)
                assert np.array_equal(area[n], np.where(want > 0, counts[want], 0)), what
                on_border = np.unique(np.concatenate([want[0], want[-1], want[:, 0], want[:, -1]]))
                assert np.array_equal(edge[n], np.isin(want, on_border[on_border > 0]).astype(np.uint8)), what
                assert np.array_equal(labels[n] > 0, fg)


def test_the_bank_is_what_it_says():
    m = CU.masks("rand0.41", (1, 130, 67))[0], CU.masks("rand0.55", (1, 130, 67))[0], CU.masks("rand0.62", (1, 130, 67))[0]
    assert [CU.scipy_count(a, 8) for a in m] == [129, 18, 6] and [CU.scipy_count(a, 4) for a in m] == [928, 404, 194]
    s = CU.masks("serpentine", (1, 131, 67))[0]
    assert s.sum() == 4487 and CU.scipy_count(s, 4) == 1 and CU.scipy_count(CU.masks("serpentine_t", (1, 67, 131))[0], 4) == 1
    c = CU.masks("checker", (1, 70, 70))[0]
    assert CU.scipy_count(c, 4) == 2450 and CU.scipy_count(c, 8) == 1
    assert CU.scipy_count(CU.masks("spiral", (1, 150, 150))[0], 4) == 1 and CU.scipy_count(~CU.masks("spiral", (1, 150, 150))[0], 4) == 1
    r = CU.masks("rings", (1, 150, 150))[0]
    assert CU.scipy_count(r, 8) > 20 and CU.scipy_count(~r, 4) > 20   # rings, and the gaps between them
    p = CU.float_bank((2, 130, 67))
    for pattern in (0x3f000000, 0x3effffff, 0x80000000, 0x7fc12345, 0x7f800000, 0xff800000, 0xffc00001):
        assert (p.view(np.uint32) == pattern).sum() > 100


def test_foreground_rule_on_special_values():
    p = np.array([[[0.5, np.nextafter(f32(0.5), f32(0)), -0.0, np.nan, np.inf, -np.inf, 0.75]]], f32)
    labels, area, edge = hostio.label_components(p, 0.5, 4)
    assert labels.tolist() == [[[1, 0, 0, 0, 5, 0, 7]]] and area.tolist() == [[[1, 0, 0, 0, 1, 0, 1]]] and edge.tolist() == [[[1, 0, 0, 0, 1, 0, 1]]]
    inv = hostio.label_components(p, 0.5, 4, invert=True)[0]
    assert inv.tolist() == [[[0, 2, 2, 2, 0, 6, 0]]]                      # NaN belongs to the complement
    for bad in (dict(threshold=np.nan), dict(threshold=np.inf), dict(connectivity=6), dict(connectivity=True)):
        kw = dict(threshold=0.5, connectivity=8)
        kw.update(bad)
        with pytest.raises(ValueError):
            hostio.label_components(p, **kw)
    with pytest.raises(ValueError):
        hostio.label_components(p[0], 0.5, 8)
    for bad in (-1, 1.5, None):
        with pytest.raises(ValueError):
            hostio.filter_components(p, 0.5, 8, bad, 0)
        with pytest.raises(ValueError):
            hostio.filter_components(p, 0.5, 8, 0, bad)


@pytest.mark.parametrize("connectivity", CU.CONNECTIVITIES)
@pytest.mark.parametrize("kind,shape", CU.FILTER_CASES, ids=CU.FILTER_IDS)
def test_filter_components_against_a_scipy_composition(kind, shape, connectivity):
    p = CU.filter_input(kind, shape)
    for min_area, max_hole in CU.FILTER_ARGS:
        out, stats = hostio.filter_components(p, CU.THRESHOLD, connectivity, min_area, max_hole)
        assert out.dtype == f32 and out.shape == p.shape and stats.dtype == np.int64 and stats.shape == (shape[0], 6)
        for n in range(shape[0]):
            want, want_stats = CU.scipy_filter(p[n], CU.THRESHOLD, connectivity, min_area, max_hole)
            assert np.array_equal(CU.bits(out[n]), CU.bits(want)), (kind, shape, connectivity, min_area, max_hole, n)
            assert np.array_equal(stats[n], want_stats), (kind, shape, connectivity, min_area, max_hole, n, stats[n], want_stats)
        if min_area <= 1:
            assert not stats[:, :3].any()
        if max_hole == 0:
            assert not stats[:, 3:].any()
        if kind == "rand0.55" and shape == (1, 150, 150) and connectivity == 8 and (min_area, max_hole) == (20, 20):
            assert stats[0, 1] == 41 and stats[0, 4] >= 1000 and (CU.bits(out) != CU.bits(p)).sum() > 2000   # the reference removes and fills
    if kind == "checker" and connectivity == 8:   # one component at 8; its one-pixel holes are the 4-connected background pixels inside
        _, stats = hostio.filter_components(p, CU.THRESHOLD, 8, 0, 1)
        assert stats[0, 3] == stats[0, 4] == stats[0, 5] == 2312
    if kind == "rings":   # a hole that holds a speck: removing the speck first makes the innermost hole one piece
        a = hostio.filter_components(p, CU.THRESHOLD, connectivity, 2, 1 << 24)[1]
        b = hostio.filter_components(p, CU.THRESHOLD, connectivity, 0, 1 << 24)[1]
        assert a[0, 1] == 1 and a[0, 2] == 1 and a[0, 5] == b[0, 5] + 1


@pytest.mark.parametrize("connectivity", CU.CONNECTIVITIES)
@pytest.mark.parametrize("shape", CU.SHAPES, ids=SHAPE_IDS)
def test_pair_count_against_scipy(shape, connectivity):
    p = CU.prob_of(CU.masks("rand0.55", shape))
    labels = CU.pair_labels(shape)
    got = hostio.components_pair_count(p, CU.THRESHOLD, labels, connectivity)
    assert got.dtype == np.int64 and got.shape == (4,)
    want = np.zeros(4, np.int64)
    for n in range(shape[0]):
        counted = (labels[n] == 0) | (labels[n] == 1)
        cp, cy = CU.scipy_count(counted & (p[n] >= f32(0.5)), connectivity), CU.scipy_count(labels[n] == 1, connectivity)
        want += (cp, cy, abs(cp - cy), int(counted.any()))
    assert np.array_equal(got, want), (got, want)
    if shape[0] > 1:   # the last image is ignored altogether: it adds exactly nothing
        assert np.array_equal(got, hostio.components_pair_count(p[:-1], CU.THRESHOLD, labels[:-1], connectivity)) and got[3] == shape[0] - 1
    none = hostio.components_pair_count(p, CU.THRESHOLD, np.full(shape, -1, np.int64), connectivity)
    assert not none.any()


# ------------------------------------------------------------------------------------------- the kernels' own steps, serially
@pytest.mark.parametrize("connectivity", CU.CONNECTIVITIES)
@pytest.mark.parametrize("tile,shape", [(4, (1, 23, 37)), (8, (1, 37, 29)), (8, (1, 1, 30)), (8, (1, 30, 1)), (64, (1, 131, 67))])
def test_the_serial_restatement_of_the_kernels_steps(tile, shape, connectivity):
    """hostio.label_components_tiled walks through what csrc/components.hip does -- runs, the unions with the row above (with the pairs
    it leaves out), tile roots, the merge levels' borders, flatten with the tile areas -- with small tiles, so that many levels and
    partial tiles cost little; a union that forgot a pair, or a level that forgot a border, shows here and not on a GPU"""
    H, W = shape[1:]
    for kind in CU.KINDS:
        m = CU.masks(kind, shape)[0]
        for mask in (m, ~m):
            labels, area, edge, levels = hostio.label_components_tiled(mask, connectivity, tile)
            want = CU.scipy_labels(mask, connectivity)
            assert np.array_equal(labels, want), (kind, tile, shape, connectivity)
            a, e = CU.scipy_area_edge(want)
            assert np.array_equal(area, a) and np.array_equal(edge, e), (kind, tile, shape, connectivity)
            t = max(-(-H // tile), -(-W // tile))
            assert levels == int(np.ceil(np.log2(t))) if t > 1 else levels == 0
