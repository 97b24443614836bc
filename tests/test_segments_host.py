"""No GPU: the tenth public header include/rsu_segments.h (road segments). The library exports what the header declares and
_lib.SIGNATURES_SEGMENTS binds exactly that, disjoint from the other nine tables; the size function against its stated layout and every
refusal with pointers nobody may follow; the 2-GiB refusal one image past the limit; tests/test_gpu_segments_fenced.py leaves no launching
entry of the header out; the flags, their parsers and refusals; the block and tile constants of tests/segments_util.py pinned to
csrc/segments.hip; hostio.line_segments on hand cases, held to scipy's labelling over the bank, and not degenerate on the thinned bank;
segment_metrics and road_graph on hand-counted inputs."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from road_segmentation_unet_amd import _lib, hostio
from road_segmentation_unet_amd import model as M
from road_segmentation_unet_amd.cli import parse_options
from tests import graph_util as GU
from tests import segments_util as SU
from tests import thin_util as TU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["rsu_line_segments", "rsu_segments_ws_bytes"]
LAUNCHING = ["rsu_line_segments"]
OLDER = ("rsu.h", "rsu_optim.h", "rsu_loss.h", "rsu_cldice.h", "rsu_lovasz.h", "rsu_components.h", "rsu_distance.h", "rsu_thin.h", "rsu_graph.h")
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
def test_library_exports_the_tenth_header_and_the_table_binds_it():
    L = _lib.lib()
    syms = _symbols("rsu_segments.h")
    assert syms == ENTRIES
    for s in syms:
        assert hasattr(L, s), "librsu_hip.so does not export %s" % s
        assert getattr(L, s).argtypes == _lib.SIGNATURES_SEGMENTS[s][1] and getattr(L, s).restype is _lib.SIGNATURES_SEGMENTS[s][0]
    assert sorted(_lib.SIGNATURES_SEGMENTS) == syms, "ctypes table and rsu_segments.h out of sync"
    tables = [set(_lib.SIGNATURES), set(_lib.SIGNATURES_OPTIM), set(_lib.SIGNATURES_LOSS), set(_lib.SIGNATURES_CLDICE),
              set(_lib.SIGNATURES_LOVASZ), set(_lib.SIGNATURES_COMPONENTS), set(_lib.SIGNATURES_DISTANCE), set(_lib.SIGNATURES_THIN),
              set(_lib.SIGNATURES_GRAPH), set(_lib.SIGNATURES_SEGMENTS)]
    for i in range(10):
        for j in range(i + 1, 10):
            assert not (tables[i] & tables[j]), (i, j)
    # the older headers' host tests look for their own substrings in every other header: none of them is in a name of this one
    assert not [n for n in syms for sub in ("thin", "dist", "components", "lovasz", "graph") if sub in n]
    assert not [n for h in OLDER for n in _symbols(h) if "segments" in n]
    assert sorted(_lib.SIGNATURES_GRAPH) == _symbols("rsu_graph.h")   # the ninth declares what it did
    assert '#include "rsu.h"' in _header("rsu_segments.h")
    for macro, value in (("RSU_SEGMENTS_MAX_SIDE", "1024"), ("RSU_SEGMENTS_MAX_EDGES", "65536")):
        assert re.search(r"^#define %s %s$" % (macro, value), _header("rsu_segments.h"), flags=re.M), macro
    assert (_lib.SEGMENTS_MAX_SIDE, _lib.SEGMENTS_MAX_EDGES) == (1024, 65536) == (hostio.SEGMENTS_MAX_SIDE, hostio.SEGMENTS_MAX_EDGES) \
        == (SU.MAX_SIDE, SU.MAX_EDGES)
    # the argument lists of the header and of the table: the same lengths, floats (by value) and ints in the same positions
    protos = _protos("rsu_segments.h")
    assert sorted(n for _, n, _ in protos) == ENTRIES
    for ret, name, args in protos:
        kinds = []
        for a in args.split(","):
            a = " ".join(a.split())
            kinds.append("f" if re.fullmatch(r"float \w+", a) else "l" if re.fullmatch(r"long \w+", a) else "i" if re.fullmatch(r"int \w+", a) else "p")
            assert kinds[-1] != "p" or "*" in a or a.startswith("rsu_stream_t "), (name, a)
        table = ["f" if t is _lib._f else "l" if t is _lib._l else "i" if t is _lib._i else "p" for t in _lib.SIGNATURES_SEGMENTS[name][1]]
        assert kinds == table, (name, kinds, table)
        assert _lib.SIGNATURES_SEGMENTS[name][0] is (_lib._sz if ret == "size_t" else _lib._i)
    # the header writes its definitions, its artefact, its launch count and what it leaves out down
    full = open(os.path.join(ROOT, "include", "rsu_segments.h")).read()
    for text in ("Z = A and dilate8(J)", "S = A \\ Z", "An L-corner is then two", "-(index + 1)", 'artefact "multi"', "8 + M",
                 "Out of scope: ordered polylines", "never on the device", "127 images, and 128 is refused"):
        assert text in full, text


def test_block_and_tile_constants_are_those_of_the_kernels():
    """the shapes and hand masks of the GPU tests are derived from these: pinned to csrc/segments.hip"""
    csrc = os.path.join(ROOT, "road_segmentation_unet_amd", "csrc")
    src = open(os.path.join(csrc, "segments.hip")).read()
    assert re.search(r"^#define SG_BLOCK %d\b" % SU.BLOCK, src, flags=re.M)
    assert re.search(r"^#define SG_TW %d\b" % SU.TILE_W, src, flags=re.M) and re.search(r"^#define SG_TH %d\b" % SU.TILE_H, src, flags=re.M)
    assert (hostio.SEGMENTS_BLOCK, hostio.SEGMENTS_TILE) == (SU.BLOCK, (SU.TILE_W, SU.TILE_H))
    assert re.search(r"^constexpr int CC_TILE = %d;" % SU.CC_TILE, open(os.path.join(csrc, "components.h")).read(), flags=re.M)
    assert [SU.launches(s) for s in SU.SHAPES] == [8, 8, 8, 9, 9, 10, 10, 12, 12]
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "$(B)/segments.o: HIPFLAGS += -ffp-contract=off" in mk and "$(B)/segments.o " in mk and "../../include/rsu_segments.h" in mk
    # the hand masks of the GPU tests: roots on the last pixel of one compaction block and the first of the next
    m = SU.block_edge_lines()
    seg = hostio.line_segments(m[None].astype(np.float32), 0.5, None, 8)[3][0]
    assert sorted(set(seg.reshape(-1).tolist()) - {0}) == [SU.BLOCK, SU.BLOCK + 1]
    # a plus whose zone (a cross of five pixels) lies across the corner of four labelling tiles: on both borders, in three of the tiles
    for c in (64, 63):
        z = hostio.segment_zones(SU.plus(128, 128, c, c, 20)[None])[1][0]
        assert z.sum() == 5 and sum(bool(q.any()) for q in (z[:64, :64], z[:64, 64:], z[64:, :64], z[64:, 64:])) == 3, c
        assert z[63].any() and z[64].any() and z[:, 63].any() and z[:, 64].any(), c


def test_size_function_and_refusals_without_a_gpu():
    L = _lib.lib()
    for shape in SU.SHAPES + [(4, 388, 388), (2, 608, 608), (1, 1024, 1024), (127, 1024, 1024)]:
        for cap in (1, 4096, 65536):
            need = L.rsu_segments_ws_bytes(*shape, cap)
            assert need == SU.ws_layout(*shape) and need % 8 == 0 and need > 0, (shape, cap)
    bad_sizes = ((0, 5, 5), (5, 0, 5), (5, 5, 0), (-1, 5, 5), (5, -1, 5), (5, 5, -1), (1, 1025, 5), (1, 5, 1025), (1, 1 << 20, 1))
    for bad in bad_sizes + ((128, 1024, 1024), (1 << 30, 2, 1)):
        assert L.rsu_segments_ws_bytes(*bad, 8) == 0, bad
    bad_caps = (0, -1, 65537, 1 << 30, -(1 << 31))
    for cap in bad_caps:
        assert L.rsu_segments_ws_bytes(2, 5, 7, cap) == 0, cap
    # refused before anything is launched or dereferenced: NULL pointers, and pointers nobody may follow
    ok = (2, 5, 7)
    # prob, threshold, labels64, max_edges, edges_pred, edges_true, counts, seg_pred, seg_true, node_pred, node_true, acc, ws
    G = L.rsu_line_segments
    assert G(None, 0.5, None, 8, None, None, None, None, None, None, None, None, None, *ok, None) == EINVAL
    assert G(None, 0.5, p, 8, p, p, p, p, p, p, p, p, p, *ok, None) == EINVAL          # prob
    assert G(p, 0.5, p, 8, p, p, p, p, p, p, p, p, None, *ok, None) == EINVAL          # ws
    assert G(p, 0.5, p, 8, p, p, None, p, p, p, p, p, p, *ok, None) == EINVAL          # counts
    assert G(p, 0.5, p, 8, None, p, p, p, p, p, p, p, p, *ok, None) == EINVAL          # edges_pred
    assert G(p, 0.5, p, 8, p, None, p, p, p, p, p, p, p, *ok, None) == EINVAL          # edges_true NULL although labels64 is given
    assert G(p, 0.5, p, 8, p, None, p, None, None, None, None, None, p, *ok, None) == EINVAL
    assert G(p, 0.5, None, 8, p, p, p, None, None, None, None, None, p, *ok, None) == EINVAL   # a *_true output without labels64
    assert G(p, 0.5, None, 8, p, None, p, None, p, None, None, None, p, *ok, None) == EINVAL
    assert G(p, 0.5, None, 8, p, None, p, None, None, None, p, None, p, *ok, None) == EINVAL
    for bad in bad_sizes:
        assert G(p, 0.5, p, 8, p, p, p, p, p, p, p, p, p, *bad, None) == EINVAL, bad
    for cap in bad_caps:
        assert G(p, 0.5, p, cap, p, p, p, p, p, p, p, p, p, *ok, None) == EINVAL, cap
    for t in (float("nan"), float("inf"), float("-inf")):
        assert G(p, t, p, 8, p, p, p, p, p, p, p, p, p, *ok, None) == EINVAL


def test_two_gib_refusal_one_image_past_the_limit():
    """at 1024 x 1024 the four int32 planes of one internal array take 16 MiB per image: 127 images are the last batch below 0x7ffffff0
    bytes, 128 reach 2 GiB; labels64 has half of that per image, so the bound is the same with and without it"""
    L = _lib.lib()
    S = 1024
    assert 127 * S * S * 16 < 0x7ffffff0 <= 128 * S * S * 16
    assert L.rsu_segments_ws_bytes(127, S, S, 4096) == SU.ws_layout(127, S, S) > 0 and L.rsu_segments_ws_bytes(128, S, S, 4096) == 0
    G = L.rsu_line_segments
    assert G(p, 0.5, p, 8, p, p, p, p, p, p, p, p, p, 128, S, S, None) == _lib.E2BIG
    assert G(p, 0.5, p, 8, p, p, p, None, None, None, None, None, p, 128, S, S, None) == _lib.E2BIG
    assert G(p, 0.5, None, 8, p, None, p, None, None, None, None, None, p, 128, S, S, None) == _lib.E2BIG    # the same bound without labels64
    assert G(p, 0.5, None, 8, p, None, p, p, None, p, None, p, p, 255, S, S, None) == _lib.E2BIG
    with pytest.raises(_lib.RsuError, match="2 GiB"):
        _lib.call("rsu_line_segments", p, 0.5, p, 8, p, p, p, p, p, p, p, p, p, 128, S, S, None)
    # a wrong argument is reported before the size
    assert G(p, float("nan"), p, 8, p, p, p, p, p, p, p, p, p, 128, S, S, None) == EINVAL
    assert G(None, 0.5, p, 8, p, p, p, p, p, p, p, p, p, 128, S, S, None) == EINVAL
    assert G(p, 0.5, p, 0, p, p, p, p, p, p, p, p, p, 128, S, S, None) == EINVAL
    assert G(p, 0.5, p, 8, p, None, p, p, p, p, p, p, p, 128, S, S, None) == EINVAL
    assert G(p, 0.5, None, 8, p, None, p, None, p, None, None, None, p, 128, S, S, None) == EINVAL


def test_the_fenced_file_covers_every_launching_entry_of_the_tenth_header():
    from tests import test_gpu_segments_fenced as G
    protos = _protos("rsu_segments.h")
    launching = [n for r, n, a in protos if r == "int" and "rsu_stream_t" in a]
    assert sorted(launching) == LAUNCHING and [n for r, n, a in protos if r == "size_t"] == ["rsu_segments_ws_bytes"]
    tests = {n: f for n, f in vars(G).items() if n.startswith("test_") and callable(f)}
    assert sorted(G.FENCED) == LAUNCHING
    for entry, names in G.FENCED.items():
        assert names, entry
        for n in names:
            assert n in tests, (entry, n)
            assert re.search(r'"%s"' % entry, inspect.getsource(tests[n]) + "".join(inspect.getsource(h) for h in G.HELPERS.get(n, ()))), \
                "%s is not launched by %s" % (entry, n)
    assert "pytest.mark.gpu" in inspect.getsource(G)
    assert "rsu_segments_ws_bytes" in inspect.getsource(G)   # exact workspaces


# ------------------------------------------------------------------------------------------- the flags and their parsers
def test_flags_defaults_parsers_and_refusals():
    defs = {d[0]: d for d in M.EXTRA_FLAG_DEFS}
    assert defs["validate_segments"][1:3] == (bool, False) and defs["max_segments"][1:3] == (int, 4096)
    assert defs["save_road_graph"][1:3] == (bool, False)
    for o in (M.Options(), parse_options([])):
        assert (o.validate_segments, o.max_segments, o.save_road_graph) == (False, 4096, False)
    o = parse_options(["--validate_centerlines", "--validate_segments", "--max_segments=100", "--centerline_min_branch=8"])
    assert (o.validate_centerlines, o.validate_segments, o.max_segments, o.centerline_min_branch) == (True, True, 100, 8)
    assert parse_options(["--validate_centerlines", "--novalidate_segments"]).validate_segments is False
    o = parse_options(["--save_road_graph", "--max_segments=65536"])         # the graph at inference needs no validation
    assert o.save_road_graph is True and o.max_segments == 65536
    assert M.parse_max_segments(1) == 1 and M.parse_max_segments("65536") == 65536
    assert isinstance(M.parse_max_segments(np.int64(3)), int) and M.parse_max_segments(4.0) == 4
    for bad in (0, -1, 65537, 1.5, float("nan"), float("inf"), "x", "", None, True, 1 << 31, (1, 2)):
        with pytest.raises(ValueError, match="max_segments"):
            M.parse_max_segments(bad)
        with pytest.raises(ValueError):
            M.Options(max_segments=bad)
    # the segments need the centre-lines: refused when the options are checked, in the constructor and on the command line
    with pytest.raises(ValueError, match="validate_centerlines"):
        M.Options(validate_segments=True)
    with pytest.raises(ValueError, match="validate_centerlines"):
        parse_options(["--validate_segments", "--validate_distances"])
    with pytest.raises(ValueError, match="validate_centerlines"):
        parse_options(["--validate_segments", "--save_road_graph", "--save_centerlines"])
    for bad in ("--max_segments=0", "--max_segments=65537"):
        with pytest.raises(ValueError):
            parse_options(["--validate_centerlines", bad])
    with pytest.raises(SystemExit):
        parse_options(["--max_segments=some"])
    # no new --save_best_metric value
    for bad in ("length_ratio", "segments_pred", "road_length_pred"):
        with pytest.raises(ValueError, match="save_best_metric"):
            M.parse_save_best_metric(bad)


# ------------------------------------------------------------------------------------------- hand cases (rows: label, pixels, ortho,
# diag, node_a, node_b, contacts, ends; index = W y + x)
def _rows(mask, cap=8):
    out = hostio.line_segments(mask[None].astype(np.float32), 0.5, None, cap, fill=SU.FILL)
    k = int(out[2][0, 0])
    assert (out[0][0, k:] == SU.FILL).all() and out[1] is None and out[4] is None and out[6] is None and not out[2][0, 2:].any()
    return out[0][0, :k].tolist(), int(out[2][0, 1]), out


def test_line_segments_hand_cases_at_nine_by_nine():
    m = np.zeros((9, 9), bool)
    m[4, 1:8] = True
    assert _rows(m)[:2] == ([[38, 7, 6, 0, -44, -38, 0, 2]], 0)
    m = np.zeros((9, 9), bool)
    m[np.arange(1, 8), np.arange(1, 8)] = True
    assert _rows(m)[:2] == ([[11, 7, 0, 6, -71, -11, 0, 2]], 0)
    m = np.zeros((9, 9), bool)
    m[4, 4] = True
    rows, nodes, out = _rows(m)
    assert (rows, nodes) == ([[41, 1, 0, 0, -41, -41, 0, 1]], 0) and out[5][0, 4, 4] == -41 and out[3][0, 4, 4] == 41
    assert _rows(GU.ring(9, 9, 2, 2, 6, 6))[:2] == ([[21, 16, 16, 0, 0, 0, 0, 0]], 0)
    m = np.zeros((9, 9), bool)
    m[4, 1:8] = m[1:8, 4] = True                                    # a plus: one node of five pixels, id 1 + (3 * 9 + 4)
    rows, nodes, out = _rows(m)
    assert nodes == 1 and rows == [[14, 2, 2, 0, -14, 32, 1, 1], [38, 2, 2, 0, -38, 32, 1, 1], [43, 2, 2, 0, -44, 32, 1, 1],
                                   [59, 2, 2, 0, -68, 32, 1, 1]]
    node = out[5][0]
    assert (node == 32).sum() == 5 and node[4, 4] == 32 and sorted(node[node < 0].tolist()) == [-68, -44, -38, -14]
    assert np.array_equal(out[3][0] > 0, m & (node <= 0))
    m = np.zeros((9, 9), bool)
    m[4, 1:8] = m[5:8, 4] = True                                    # a T: the node is row 4's three pixels and the stem's first
    rows, nodes, out = _rows(m)
    assert nodes == 1 and rows == [[38, 2, 2, 0, -38, 40, 1, 1], [43, 2, 2, 0, -44, 40, 1, 1], [59, 2, 2, 0, -68, 40, 1, 1]]
    assert (out[5][0] == 40).sum() == 4
    assert np.array_equal(out[7], [[3, 6, 6, 0, 3, 0, 0, 0], [0] * 8])


def test_line_segments_corner_and_loop_with_a_tail():
    m = np.zeros((9, 12), bool)
    m[2, 1:5] = m[2:7, 4] = True                                    # an L-corner: two orthogonal links at the corner, not three
    rows, nodes, _ = _rows(m)
    assert nodes == 0 and len(rows) == 1 and rows[0][1:4] == [8, 7, 0] and rows[0][6:] == [0, 2]
    m = GU.ring(12, 12, 2, 2, 8, 8)
    m[5, 8:12] = True                                               # a loop through one node, and a dangling tail
    rows, nodes, out = _rows(m)
    assert nodes == 1 and rows == [[27, 21, 22, 0, 57, 57, 2, 0], [71, 2, 2, 0, -72, 57, 1, 1]]
    assert np.array_equal(out[7][0], [2, 23, 24, 0, 1, 0, 0, 0])
    # a diagonal contact: a diagonal line into a horizontal one's junction zone from one pixel out
    m = np.zeros((12, 12), bool)
    m[6, 1:11] = True
    m[np.arange(1, 6), np.arange(1, 6)] = True                      # ends at (5, 5), diagonal to (6, 6) and above (6, 5)
    rows, nodes, out = _rows(m)
    assert nodes == 1 and sum(r[3] for r in rows) > 0 and all(r[6] + r[7] == 2 for r in rows)
    # truncation: the first rows, the fill behind them, the true counts, acc over the stored rows
    full = _rows(SU.plus(9, 9, 4, 4, 3))[2]
    cut = hostio.line_segments(SU.plus(9, 9, 4, 4, 3)[None].astype(np.float32), 0.5, None, 3, fill=SU.FILL)
    assert np.array_equal(cut[0][0], full[0][0, :3]) and np.array_equal(cut[2], full[2]) and cut[7][0, 0] == 3 and full[7][0, 0] == 4
    for bad in (0, 65537, 1.5, True, None, "8"):
        with pytest.raises(ValueError, match="max_edges"):
            hostio.line_segments(m[None].astype(np.float32), 0.5, None, bad)
    with pytest.raises(ValueError):
        hostio.line_segments(m[None].astype(np.float32), float("nan"), None, 8)
    with pytest.raises(ValueError):
        hostio.line_segments(np.zeros((1, 4, 1025), np.float32), 0.5, None, 8)


# ------------------------------------------------------------------------------------------- invariants over the bank
HOST_SHAPE = (2, 70, 83)


@pytest.mark.parametrize("L", SU.PRUNES)
def test_line_segments_invariants_over_the_bank(L):
    from scipy import ndimage
    eight = np.ones((3, 3), int)
    for name in TU.pair_names():
        prob, labels = SU.pair(name, HOST_SHAPE, L)
        out = SU.host(prob, labels)
        ep, et, counts, sp, st, npd, nt, acc = out
        P, T = prob >= np.float32(0.5), labels == 1
        for side, (a, edges, seg, node) in enumerate(((P, ep, sp, npd), (T, et, st, nt))):
            s, z = hostio.segment_zones(a)
            assert np.array_equal(seg > 0, s) and np.array_equal(node > 0, z) and not (s & z).any() and np.array_equal(s | z, a), name
            for n in range(a.shape[0]):
                k, nodes = int(counts[n, 2 * side]), int(counts[n, 2 * side + 1])
                assert k <= SU.CAP and int(edges[n, :k, 1].sum()) == int(s[n].sum()), (name, side, n)
                lab, found = ndimage.label(s[n], structure=eight)
                assert found == k and ndimage.label(z[n], structure=eight)[1] == nodes, (name, side, n)
                if k:   # every label is 1 + the smallest row-major index of its component, and the rows ascend
                    first = np.asarray(ndimage.minimum(np.arange(s[n].size).reshape(s[n].shape), lab, index=np.arange(1, k + 1)), np.int64)
                    assert np.array_equal(np.sort(first + 1), edges[n, :k, 0]) and np.array_equal(seg[n][s[n]], (first + 1)[lab[s[n]] - 1])
                ends = node[n] < 0
                assert int(edges[n, :k, 7].sum()) == int(ends.sum()) and np.array_equal(-node[n][ends] - 1, np.flatnonzero(ends.reshape(-1)))
        # a stack gives what its images give alone
        for n in range(prob.shape[0]):
            one = hostio.line_segments(prob[n:n + 1], 0.5, labels[n:n + 1], SU.CAP, fill=SU.FILL)
            for a, b in zip(one[:7], out[:7]):
                assert np.array_equal(a[0], b[n]), name
        assert np.array_equal(acc, sum(hostio.line_segments(prob[n:n + 1], 0.5, labels[n:n + 1], SU.CAP)[7] for n in range(prob.shape[0])))


@pytest.mark.parametrize("kind", ["smooth1.5", "smooth3", "smooth6"])
def test_the_definition_is_not_degenerate_on_the_thinned_bank(kind):
    """segments, nodes and diagonal links exist, and at most 3 % of the segments are "multi": a condition on the definition (with J
    alone as the node about 30 % of the components touch four or more nodes)"""
    for shape in ((2, 64, 64), (2, 230, 97)):
        for L in SU.PRUNES:
            a = hostio.prune_mask(GU.thinned(kind, shape), L)
            ep, _, counts, _, _, _, _, acc = hostio.line_segments(a.astype(np.float32), 0.5, None, 4096)
            rows, multi = int(acc[0, 0]), int(acc[0, 7])
            print(kind, shape, L, "segments", rows, "nodes", int(counts[:, 1].sum()), "diag", int(acc[0, 3]), "multi", multi)
            assert rows == counts[:, 0].sum() > 0 and counts[:, 1].sum() > 0, (kind, shape, L)
            assert (ep[..., 3] > 0).any() and acc[0, 3] > 0, (kind, shape, L)
            assert multi <= 0.03 * rows, (kind, shape, L, multi, rows)
    if kind == "smooth1.5":
        a = hostio.prune_mask(GU.thinned(kind, (2, 64, 64)), 8)
        acc = hostio.line_segments(a.astype(np.float32), 0.5, None, 4096)[7]
        assert acc[0].tolist() == [74, 538, 319, 249, 44, 0, 0, 1]


# ------------------------------------------------------------------------------------------- segment_metrics, road_graph
def test_segment_metrics_hand_counted():
    acc = np.array([[10, 100, 60, 30, 3, 1, 1, 1], [8, 90, 50, 20, 2, 0, 0, 0]], np.int64)
    m = hostio.segment_metrics(acc, np.array([12, 5, 8, 4], np.int64))
    r2 = float(np.sqrt(np.float64(2.0)))
    lp, lt = 60 + r2 * 30, 50 + r2 * 20
    assert m == {"segments_pred": 10, "road_length_pred": lp, "seg_len_mean_pred": lp / 10, "dangling_pred": 3, "free_pred": 1, "rings_pred": 1,
                 "multi_pred": 1, "segments_dropped_pred": 2, "nodes_pred": 5,
                 "segments_true": 8, "road_length_true": lt, "seg_len_mean_true": lt / 8, "dangling_true": 2, "free_true": 0, "rings_true": 0,
                 "multi_true": 0, "segments_dropped_true": 0, "nodes_true": 4, "length_ratio": lp / lt}
    empty = hostio.segment_metrics(np.zeros((2, 8), np.int64), np.zeros(4, np.int64))
    assert set(empty) == set(m) and not any(empty.values())
    for bad in (np.zeros(16, np.int64), np.zeros((2, 8), np.float64), -np.ones((2, 8), np.int64)):
        with pytest.raises(ValueError, match="acc"):
            hostio.segment_metrics(bad, np.zeros(4, np.int64))
    for bad in (np.zeros(3, np.int64), np.zeros(4, np.float64), np.array([1, -1, 1, 1]), 5):
        with pytest.raises(ValueError, match="counts_sum"):
            hostio.segment_metrics(acc, bad)
    with pytest.raises(ValueError, match="stored rows"):
        hostio.segment_metrics(acc, np.array([9, 5, 8, 4], np.int64))


def test_road_graph_hand_counted():
    m = GU.ring(12, 12, 2, 2, 8, 8)
    m[5, 8:12] = True
    m[10, 1] = True                                                  # and an isolated pixel
    out = hostio.line_segments(m[None].astype(np.float32), 0.5, None, 8)
    g = hostio.road_graph(out[0][0], int(out[2][0, 0]), out[5][0], 12, 12)
    assert g["nodes"] == [{"id": -122, "kind": "isolated", "y": 10.0, "x": 1.0}, {"id": -72, "kind": "end", "y": 5.0, "x": 11.0},
                          {"id": 57, "kind": "junction", "y": 5.0, "x": 8.25}]
    assert g["edges"] == [{"id": 27, "a": 57, "b": 57, "pixels": 21, "length": 22.0, "contacts": 2, "ends": 0},
                          {"id": 71, "a": -72, "b": 57, "pixels": 2, "length": 2.0, "contacts": 1, "ends": 1},
                          {"id": 122, "a": -122, "b": -122, "pixels": 1, "length": 0.0, "contacts": 0, "ends": 1}]
    d = np.zeros((9, 9), bool)
    d[np.arange(1, 8), np.arange(1, 8)] = True
    out = hostio.line_segments(d[None].astype(np.float32), 0.5, None, 8)
    g = hostio.road_graph(out[0][0], 1, out[5][0], 9, 9)
    assert g["edges"][0]["length"] == 6 * float(np.sqrt(np.float64(2.0))) and [n["kind"] for n in g["nodes"]] == ["end", "end"]
    assert hostio.road_graph(out[0][0], 0, np.zeros((9, 9), np.int32), 9, 9) == {"nodes": [], "edges": []}
    import json
    assert json.loads(json.dumps(g)) == g                             # plain: it goes to a JSON file as it is
    for bad in (np.zeros((3, 7), np.int32), np.zeros((3, 8), np.float32), np.zeros(8, np.int32)):
        with pytest.raises(ValueError, match="edges"):
            hostio.road_graph(bad, 1, out[5][0], 9, 9)
    with pytest.raises(ValueError, match="node_map"):
        hostio.road_graph(out[0][0], 1, out[5][0], 9, 8)
    for bad in (-1, 1.0, True, None):
        with pytest.raises(ValueError, match="count"):
            hostio.road_graph(out[0][0], bad, out[5][0], 9, 9)
