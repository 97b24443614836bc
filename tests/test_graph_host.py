"""No GPU: the ninth public header include/rsu_graph.h (centre-line pruning and nodes). The library exports what the header declares and
_lib.SIGNATURES_GRAPH binds exactly that, disjoint from the other eight tables; the size function against its stated layout and every
refusal with pointers nobody may follow; the 2-GiB refusal one image past the limit; tests/test_gpu_graph_fenced.py leaves no launching
entry of the header out; the flags, their parsers and refusals; the tile constants of tests/graph_util.py pinned to csrc/graph.h;
hostio.prune_mask held to the topology of its input by scipy over the bank of tests/thin_util.py, raw and thinned; hand cases (free lines,
a line with spurs, a ring, a one-pixel bump); skeleton_nodes and graph_metrics on hand-counted cases; and that pruning is not trivial on
the thinned bank."""
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
from tests import thin_util as TU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["rsu_graph_ws_bytes", "rsu_skeleton_graph"]
LAUNCHING = ["rsu_skeleton_graph"]
OLDER = ("rsu.h", "rsu_optim.h", "rsu_loss.h", "rsu_cldice.h", "rsu_lovasz.h", "rsu_components.h", "rsu_distance.h", "rsu_thin.h")
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
def test_library_exports_the_ninth_header_and_the_table_binds_it():
    L = _lib.lib()
    syms = _symbols("rsu_graph.h")
    assert syms == ENTRIES
    for s in syms:
        assert hasattr(L, s), "librsu_hip.so does not export %s" % s
        assert getattr(L, s).argtypes == _lib.SIGNATURES_GRAPH[s][1] and getattr(L, s).restype is _lib.SIGNATURES_GRAPH[s][0]
    assert sorted(_lib.SIGNATURES_GRAPH) == syms, "ctypes table and rsu_graph.h out of sync"
    tables = [set(_lib.SIGNATURES), set(_lib.SIGNATURES_OPTIM), set(_lib.SIGNATURES_LOSS), set(_lib.SIGNATURES_CLDICE),
              set(_lib.SIGNATURES_LOVASZ), set(_lib.SIGNATURES_COMPONENTS), set(_lib.SIGNATURES_DISTANCE), set(_lib.SIGNATURES_THIN),
              set(_lib.SIGNATURES_GRAPH)]
    for i in range(9):
        for j in range(i + 1, 9):
            assert not (tables[i] & tables[j]), (i, j)
    # the older headers' host tests look for their own substrings in every other header: none of them is in a name of this one
    assert not [n for n in syms for sub in ("thin", "dist", "components") if sub in n]
    assert not [n for h in OLDER for n in _symbols(h) if "graph" in n]
    assert sorted(_lib.SIGNATURES_THIN) == _symbols("rsu_thin.h")   # the eighth declares what it did
    assert '#include "rsu.h"' in _header("rsu_graph.h")
    for macro, value in (("RSU_GRAPH_MAX_SIDE", "1024"), ("RSU_GRAPH_MAX_BRANCH", "64")):
        assert re.search(r"^#define %s %s$" % (macro, value), _header("rsu_graph.h"), flags=re.M), macro
    assert (_lib.GRAPH_MAX_SIDE, _lib.GRAPH_MAX_BRANCH) == (1024, 64) == (hostio.GRAPH_MAX_SIDE, hostio.GRAPH_MAX_BRANCH) \
        == (GU.MAX_SIDE, GU.MAX_BRANCH)
    # the argument lists of the header and of the table: the same lengths, floats (by value) and ints in the same positions
    protos = _protos("rsu_graph.h")
    assert sorted(n for _, n, _ in protos) == ENTRIES
    for ret, name, args in protos:
        kinds = []
        for a in args.split(","):
            a = " ".join(a.split())
            kinds.append("f" if re.fullmatch(r"float \w+", a) else "l" if re.fullmatch(r"long \w+", a) else "i" if re.fullmatch(r"int \w+", a) else "p")
            assert kinds[-1] != "p" or "*" in a or a.startswith("rsu_stream_t "), (name, a)
        table = ["f" if t is _lib._f else "l" if t is _lib._l else "i" if t is _lib._i else "p" for t in _lib.SIGNATURES_GRAPH[name][1]]
        assert kinds == table, (name, kinds, table)
        assert _lib.SIGNATURES_GRAPH[name][0] is (_lib._sz if ret == "size_t" else _lib._i)
    # the header writes its known artefact and its launch count down
    full = open(os.path.join(ROOT, "include", "rsu_graph.h")).read()
    assert "KNOWN ARTEFACT" in full and "2 + ceil(L / R) + ceil((L + 1) / R)" in full and "out_pred == prob" in full


def test_tile_constants_are_those_of_the_kernels():
    """the shapes and min_branch values of the GPU tests are derived from these: pinned to csrc/graph.h and csrc/graph.hip"""
    csrc = os.path.join(ROOT, "road_segmentation_unet_amd", "csrc")
    src = open(os.path.join(csrc, "graph.h")).read() + open(os.path.join(csrc, "graph.hip")).read()
    assert re.search(r"^#define GR_R %d$" % GU.R, src, flags=re.M) and re.search(r"^#define GR_ROWS %d\b" % (GU.CROWS + 2 * GU.R), src, flags=re.M)
    assert "GR_HALO = GR_R;" in src and "GR_CORE = 64 - 2 * GR_HALO;" in src and GU.CORE == 64 - 2 * GU.R
    assert GU.BRANCHES == (0, 1, 15, 16, 17, 33, 64)
    assert [GU.launches(L) for L in GU.BRANCHES] == [2, 4, 4, 5, 6, 8, 11]
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "$(B)/graph.o: HIPFLAGS += -ffp-contract=off" in mk and "$(B)/graph.o " in mk and "../../include/rsu_graph.h" in mk
    # the hand-drawn masks of the GPU tests lie across the corner of four tiles
    line, ring = GU.corner_line()[0], GU.corner_ring()[0]
    assert line[GU.CROWS - 1].all() and line[GU.CROWS:, :].any() and line[:GU.CROWS - 1].any()
    assert sorted(set(int(line[:, x].sum()) - 1 for x in range(line.shape[1])) - {0}) == list(range(1, 2 * GU.R + 3))
    for m in (line, ring):
        for y, x in ((GU.CROWS, GU.CORE), (GU.CROWS, 2 * GU.CORE), (GU.CROWS, 3 * GU.CORE)):
            assert m[:y, :x].any() and m[:y, x:].any() and m[y:, :x].any() and m[y:, x:].any()


def _ws(N, H, W, L):
    """the layout of csrc/graph.hip: one bit plane of [N][2][H][ceil(W / CORE)] 64-bit words without a prune phase, five with one, then
    [ceil(L / R) + ceil((L + 1) / R)][N][2] counters"""
    steps = (-(-L // GU.R) + -(-(L + 1) // GU.R)) if L else 0
    return (5 if L else 1) * N * 2 * H * (-(-W // GU.CORE)) * 8 + -(-(steps * N * 2 * 4) // 8) * 8


def test_size_function_and_refusals_without_a_gpu():
    L = _lib.lib()
    for shape in GU.SHAPES + [GU.CORNER_SHAPE, (4, 388, 388), (2, 608, 608), (1, 1024, 1024), (255, 1024, 1024), (511, 1024, 1024)]:
        for b in GU.BRANCHES + (2, 8, 63):
            need = L.rsu_graph_ws_bytes(*shape, b)
            assert need == _ws(*shape, b) and need % 8 == 0 and need > 0, (shape, b)
    bad_sizes = ((0, 5, 5), (5, 0, 5), (5, 5, 0), (-1, 5, 5), (5, -1, 5), (5, 5, -1), (1, 1025, 5), (1, 5, 1025), (1, 1 << 20, 1))
    for bad in bad_sizes + ((512, 1024, 1024), (1 << 30, 2, 1)):
        assert L.rsu_graph_ws_bytes(*bad, 8) == 0, bad
    for b in (-1, 65, 1 << 30):
        assert L.rsu_graph_ws_bytes(2, 5, 7, b) == 0, b
    # refused before anything is launched or dereferenced: NULL pointers, and pointers nobody may follow
    ok = (2, 5, 7)
    # prob, threshold, labels64, min_branch, out_pred, out_true, junc_pred, junc_true, acc, ws
    G = L.rsu_skeleton_graph
    assert G(None, 0.5, None, 8, None, None, None, None, None, None, *ok, None) == EINVAL
    assert G(None, 0.5, p, 8, p, p, p, p, p, p, *ok, None) == EINVAL            # prob
    assert G(p, 0.5, p, 8, p, p, p, p, p, None, *ok, None) == EINVAL            # ws
    assert G(p, 0.5, p, 8, None, None, None, None, p, p, *ok, None) == EINVAL   # no output at all
    assert G(p, 0.5, None, 8, None, None, None, None, None, p, *ok, None) == EINVAL
    assert G(p, 0.5, None, 8, p, p, None, None, None, p, *ok, None) == EINVAL   # a *_true output without labels
    assert G(p, 0.5, None, 8, None, p, None, None, None, p, *ok, None) == EINVAL
    assert G(p, 0.5, None, 8, p, None, p, p, None, p, *ok, None) == EINVAL
    assert G(p, 0.5, None, 8, None, None, None, p, p, p, *ok, None) == EINVAL
    for bad in bad_sizes:
        assert G(p, 0.5, p, 8, p, p, p, p, p, p, *bad, None) == EINVAL, bad
    for b in (-1, 65, 1 << 30, -(1 << 31)):
        assert G(p, 0.5, p, b, p, p, p, p, p, p, *ok, None) == EINVAL, b
    for t in (float("nan"), float("inf"), float("-inf")):
        assert G(p, t, p, 8, p, p, p, p, p, p, *ok, None) == EINVAL


def test_two_gib_refusal_one_image_past_the_limit():
    """at 1024 x 1024 labels64 and the *_true outputs take 8 MiB per image: 255 images are the last batch below 0x7ffffff0 bytes, 256 reach
    2 GiB. Without labels64 the largest tensor has 4 bytes per pixel: 511 images pass, 512 do not."""
    L = _lib.lib()
    S = 1024
    assert 255 * S * S * 8 < 0x7ffffff0 <= 256 * S * S * 8 and 511 * S * S * 4 < 0x7ffffff0 <= 512 * S * S * 4
    assert L.rsu_graph_ws_bytes(255, S, S, 8) == _ws(255, S, S, 8) > 0 and L.rsu_graph_ws_bytes(511, S, S, 0) == _ws(511, S, S, 0) > 0
    G = L.rsu_skeleton_graph
    assert G(p, 0.5, p, 8, p, p, p, p, p, p, 256, S, S, None) == _lib.E2BIG
    assert G(p, 0.5, p, 8, None, p, None, None, None, p, 256, S, S, None) == _lib.E2BIG
    assert G(p, 0.5, p, 8, p, None, None, None, None, p, 256, S, S, None) == _lib.E2BIG    # labels64 given: it is the largest tensor
    assert G(p, 0.5, None, 8, p, None, None, None, None, p, 512, S, S, None) == _lib.E2BIG
    assert G(p, 0.5, None, 0, None, None, p, None, None, p, 512, S, S, None) == _lib.E2BIG
    with pytest.raises(_lib.RsuError, match="2 GiB"):
        _lib.call("rsu_skeleton_graph", p, 0.5, p, 8, p, p, p, p, p, p, 256, S, S, None)
    # a wrong argument is reported before the size
    assert G(p, float("nan"), p, 8, p, p, p, p, p, p, 256, S, S, None) == EINVAL
    assert G(None, 0.5, p, 8, p, p, p, p, p, p, 256, S, S, None) == EINVAL
    assert G(p, 0.5, p, 65, p, p, p, p, p, p, 256, S, S, None) == EINVAL


def test_the_fenced_file_covers_every_launching_entry_of_the_ninth_header():
    from tests import test_gpu_graph_fenced as G
    protos = _protos("rsu_graph.h")
    launching = [n for r, n, a in protos if r == "int" and "rsu_stream_t" in a]
    assert sorted(launching) == LAUNCHING and [n for r, n, a in protos if r == "size_t"] == ["rsu_graph_ws_bytes"]
    tests = {n: f for n, f in vars(G).items() if n.startswith("test_") and callable(f)}
    assert sorted(G.FENCED) == LAUNCHING
    for entry, names in G.FENCED.items():
        assert names, entry
        for n in names:
            assert n in tests, (entry, n)
            assert re.search(r'"%s"' % entry, inspect.getsource(tests[n]) + "".join(inspect.getsource(h) for h in G.HELPERS.get(n, ()))), \
                "%s is not launched by %s" % (entry, n)
    assert "pytest.mark.gpu" in inspect.getsource(G)
    assert "rsu_graph_ws_bytes" in inspect.getsource(G)   # exact workspaces


# ------------------------------------------------------------------------------------------- the flags and their parsers
def test_flags_defaults_parsers_and_refusals():
    defs = {d[0]: d for d in M.EXTRA_FLAG_DEFS}
    assert defs["centerline_min_branch"][1:3] == (int, 0) and defs["validate_junctions"][1:3] == (bool, False)
    assert "cldice_hard stays on the unpruned" in defs["centerline_min_branch"][3] and "ends there" in defs["validate_junctions"][3]
    for o in (M.Options(), parse_options([])):
        assert (o.centerline_min_branch, o.validate_junctions) == (0, False)
    o = parse_options(["--validate_centerlines", "--centerline_min_branch=8", "--validate_junctions"])
    assert (o.validate_centerlines, o.centerline_min_branch, o.validate_junctions) == (True, 8, True)
    assert parse_options(["--validate_centerlines", "--novalidate_junctions"]).validate_junctions is False
    assert parse_options(["--save_centerlines", "--centerline_min_branch=64"]).centerline_min_branch == 64   # pruning alone needs no validation
    assert M.parse_centerline_min_branch(0) == 0 and M.parse_centerline_min_branch("64") == 64
    assert isinstance(M.parse_centerline_min_branch(np.int64(3)), int) and M.parse_centerline_min_branch(4.0) == 4
    for bad in (-1, 65, 1.5, float("nan"), float("inf"), "x", "", None, True, 1 << 31, (1, 2)):
        with pytest.raises(ValueError, match="centerline_min_branch"):
            M.parse_centerline_min_branch(bad)
        with pytest.raises(ValueError):
            M.Options(centerline_min_branch=bad)
    # the junctions need the centre-lines: refused when the options are checked, in the constructor and on the command line
    with pytest.raises(ValueError, match="validate_centerlines"):
        M.Options(validate_junctions=True)
    with pytest.raises(ValueError, match="validate_centerlines"):
        parse_options(["--validate_junctions", "--validate_distances"])
    with pytest.raises(ValueError, match="validate_centerlines"):
        parse_options(["--validate_junctions", "--centerline_min_branch=3", "--save_centerlines"])
    for bad in ("--centerline_min_branch=-1", "--centerline_min_branch=65"):
        with pytest.raises(ValueError):
            parse_options(["--validate_centerlines", bad])
    with pytest.raises(SystemExit):
        parse_options(["--centerline_min_branch=some"])
    # no new --save_best_metric value
    for bad in ("jn_f1", "junction_error"):
        with pytest.raises(ValueError, match="save_best_metric"):
            M.parse_save_best_metric(bad)


# ------------------------------------------------------------------------------------------- prune_mask: the topology of its input
HOST_SHAPE = (2, 70, 83)
BIG_SHAPE = (1, 130, 133)
HOST_BRANCHES = (1, 3, 8, 20)


def _check_pruned(a, b, what):
    """B inside A; the 4-connected background of A unchanged in number (no loop opened, none closed); no 8-component of A holds two
    components of B (nothing is cut in two)"""
    from scipy import ndimage
    assert b.dtype == np.bool_ and b.shape == a.shape and not (b & ~a).any(), what
    eight = np.ones((3, 3), int)
    for n in range(a.shape[0]):
        assert TU.topology(b[n])[1] == TU.topology(a[n])[1], (what, n, "background")
        lab_a = ndimage.label(a[n], structure=eight)[0]
        lab_b, k = ndimage.label(b[n], structure=eight)
        if k:
            owner = np.asarray(ndimage.maximum(lab_a, lab_b, index=np.arange(1, k + 1)), np.int64)
            assert len(set(owner.tolist())) == k, (what, n, "a component of A holds two of B")


@pytest.mark.parametrize("kind", TU.KINDS)
def test_prune_mask_keeps_the_topology_of_its_input(kind):
    for shape in (HOST_SHAPE, BIG_SHAPE):
        for a in (TU.masks(kind, shape), GU.thinned(kind, shape)):
            assert np.array_equal(hostio.prune_mask(a, 0), a)
            for L in HOST_BRANCHES:
                b = hostio.prune_mask(a, L)
                _check_pruned(a, b, (kind, shape, L))


def test_prune_mask_hand_cases():
    # free lines, straight and diagonal: 2 L pixels vanish, 2 L + 1 and 2 L + 2 return whole
    for L in (1, 3, 8):
        for n, stays in ((2 * L, False), (2 * L + 1, True), (2 * L + 2, True)):
            m = np.zeros((2, 30, 40), bool)
            m[0, 2, 3:3 + n] = True
            m[1][np.arange(2, 2 + n), np.arange(5, 5 + n)] = True
            b = hostio.prune_mask(m, L)
            assert np.array_equal(b, m) if stays else not b.any(), (L, n)
    # a line of 65 pixels with spurs of 1 .. 6 pixels at L = 3: spurs 2 and 3 go, 4 to 6 stay whole; spur 1 stands two pixels from the
    # line's end and returns with it -- the artefact include/rsu_graph.h documents
    spurs = [1, 2, 3, 4, 5, 6]
    m = GU.line_with_spurs(21, 70, 10, 2, 66, spurs, step=9, first=4)
    b = hostio.prune_mask(m[None], 3)[0]
    assert b[10, 2:67].all() and b[10].sum() == 65
    left = [int(b[:, 4 + 9 * k].sum()) - 1 for k in range(6)]
    assert left == [1, 0, 0, 4, 5, 6]
    far = GU.line_with_spurs(21, 70, 10, 2, 66, [1], step=9, first=30)    # the same spur far from both ends goes
    assert np.array_equal(hostio.prune_mask(far[None], 3)[0], GU.line_with_spurs(21, 70, 10, 2, 66, [], step=9))
    ends, iso, junc = hostio.skeleton_nodes(b[None])
    assert ends.sum() == 2 + 3 + 1 and not iso.any() and junc.sum() >= 4
    # a closed loop is untouched at every L, and has no node
    ring = GU.ring(20, 24, 3, 3, 12, 15)[None]
    for L in (1, 8, 64):
        assert np.array_equal(hostio.prune_mask(ring, L), ring)
    assert not any(a.any() for a in hostio.skeleton_nodes(ring))
    # a one-pixel bump on a line: a false junction before, none after one round; the line is whole
    bump = np.zeros((1, 7, 20), bool)
    bump[0, 3, 1:19] = True
    line = bump.copy()
    bump[0, 2, 9] = True
    assert hostio.skeleton_nodes(bump)[2].sum() == 1
    b = hostio.prune_mask(bump, 1)
    assert np.array_equal(b, line) and not hostio.skeleton_nodes(b)[2].any() and hostio.skeleton_nodes(b)[0].sum() == 2
    # images are independent: a stack gives what its images give alone
    stack = GU.thinned("smooth3", HOST_SHAPE)
    both = hostio.prune_mask(stack, 8)
    assert all(np.array_equal(hostio.prune_mask(stack[n:n + 1], 8)[0], both[n]) for n in range(2))
    for bad in (np.zeros((4, 4), bool), np.zeros((1, 4, 4), np.uint8), np.zeros((1, 0, 4), bool)):
        with pytest.raises(ValueError, match="prune_mask"):
            hostio.prune_mask(bad, 8)
        with pytest.raises(ValueError, match="skeleton_nodes"):
            hostio.skeleton_nodes(bad)
    for bad in (-1, 65, 1.5, True, None, "8"):
        with pytest.raises(ValueError, match="min_branch"):
            hostio.prune_mask(np.zeros((1, 4, 4), bool), bad)


def test_skeleton_nodes_hand_counted():
    m = np.zeros((4, 9, 9), bool)
    m[0, 4, 1:8] = True                      # a line: two ends
    m[1, 4, 1:8] = m[1, 1:8, 4] = True       # a plus: four ends; its centre has X = 4
    m[2, 4, 4] = True                        # a lone pixel
    m[2, 0, 0] = m[2, 0, 1] = True           # two pixels in the corner: two ends (everything outside the image is background)
    m[3, 4, 1:8] = m[3, 5:8, 4] = True       # a T: three ends; the centre has X = 3
    ends, iso, junc = hostio.skeleton_nodes(m)
    assert [int(a.sum()) for a in ends] == [2, 4, 2, 3] and [int(a.sum()) for a in iso] == [0, 0, 1, 0]
    assert ends[0, 4, 1] and ends[0, 4, 7] and iso[2, 4, 4] and ends[2, 0, 0] and ends[2, 0, 1]
    assert [int(a.sum()) for a in junc] == [0, 1, 0, 1] and junc[1, 4, 4] and junc[3, 4, 4]
    # a solid 3 x 3 block: no pixel has a crossing number above 1, the corners are ENDs (one run of three neighbours), the rest is not
    blk = np.zeros((1, 7, 7), bool)
    blk[0, 2:5, 2:5] = True
    e, i, j = hostio.skeleton_nodes(blk)
    assert e.sum() == 4 and not i.any() and not j.any()
    # a diagonal crossing (an X): the centre has four runs
    x = np.zeros((1, 7, 7), bool)
    x[0][np.arange(7), np.arange(7)] = x[0][np.arange(7), 6 - np.arange(7)] = True
    e, i, j = hostio.skeleton_nodes(x)
    assert e.sum() == 4 and j.sum() == 1 and j[0, 3, 3]


def test_skeleton_graph_formats_and_counts():
    shape = (3, 63, 65)
    from tests import components_util as CU
    prob, labels = CU.float_bank(shape), TU.mixed_labels(shape)
    op, ot, jp, jt, counts = hostio.skeleton_graph(prob, 0.5, labels, 3)
    counted = (labels == 0) | (labels == 1)
    with np.errstate(invalid="ignore"):
        P, T = (prob >= np.float32(0.5)) & counted, labels == 1
    assert op.dtype == jp.dtype == np.float32 and ot.dtype == jt.dtype == np.int64 and counts.dtype == np.int64 and counts.shape == (8,)
    BP, BT = hostio.prune_mask(P, 3), hostio.prune_mask(T, 3)
    assert set(np.unique(op)) <= {0.0, 1.0} and np.array_equal(op > 0, BP) and np.array_equal(jp > 0, hostio.skeleton_nodes(BP)[2])
    for got, want in ((ot, BT), (jt, hostio.skeleton_nodes(BT)[2])):
        assert np.array_equal(got[~counted], labels[~counted]) and np.array_equal(got[counted] == 1, want[counted])
    nodes = [hostio.skeleton_nodes(b) for b in (BP, BT)]
    assert list(counts) == [BP.sum()] + [a.sum() for a in nodes[0]] + [BT.sum()] + [a.sum() for a in nodes[1]]
    # (an isolated pixel is a free curve of one pixel: any L > 0 takes it; only an unpruned mask has some)
    assert (counts[[0, 1, 3, 4, 5, 7]] > 0).all() and counts[2] == counts[6] == 0 and hostio.skeleton_graph(prob, 0.5, labels, 0)[4].min() > 0
    assert not op[-1].any() and (ot[-1] == -1).all() and (jt[-1] == -1).all()      # the all-ignored image
    assert np.array_equal(hostio.skeleton_graph(prob[:-1], 0.5, labels[:-1], 3)[4], counts)
    # min_branch 0: the masks themselves; the entry takes mask_thin's outputs as they are
    sp, st, _, _ = hostio.mask_thin(prob, 0.5, labels, 64)
    same = hostio.skeleton_graph(sp, 0.5, st, 0)
    assert same[0].tobytes() == sp.tobytes() and same[1].tobytes() == st.tobytes()
    free = hostio.skeleton_graph(prob, 0.5, None, 3)
    assert free[1] is None and free[3] is None and not free[4][4:].any() and free[4][0] > 0
    with pytest.raises(ValueError):
        hostio.skeleton_graph(prob, float("nan"), labels, 3)
    with pytest.raises(ValueError):
        hostio.skeleton_graph(prob, 0.5, labels[:2], 3)
    with pytest.raises(ValueError, match="min_branch"):
        hostio.skeleton_graph(prob, 0.5, labels, 65)


# ------------------------------------------------------------------------------------------- graph_metrics
def test_graph_metrics_hand_counted():
    h = np.zeros((2, 64), np.int64)
    h[0, :4] = (3, 2, 1, 1)      # ten predicted junction pixels: 3 on a true one, 2 one pixel off, ... and three far from any
    h[0, 63] = 3
    h[1, :3] = (3, 4, 1)
    counts = np.array([100, 9, 1, 10, 90, 7, 0, 8], np.int64)
    m = hostio.graph_metrics(h, [4, 3, 5, 4], counts, 1)
    prec, rec = 5 / 10, 7 / 8
    assert m == {"jn_precision": prec, "jn_recall": rec, "jn_f1": 2 * prec * rec / (prec + rec), "junctions_pred": 4, "junctions_true": 3,
                 "junction_error": 5 / 4, "ends_pred": 9, "ends_true": 7, "isolated_pred": 1, "isolated_true": 0}
    m0 = hostio.graph_metrics(h, [4, 3, 5, 4], counts, 0)
    assert (m0["jn_precision"], m0["jn_recall"]) == (3 / 10, 3 / 8)
    empty = hostio.graph_metrics(np.zeros((2, 64), np.int64), np.zeros(4, np.int64), np.zeros(8, np.int64), 3)
    assert empty == {"jn_precision": 0.0, "jn_recall": 0.0, "jn_f1": 0.0, "junctions_pred": 0, "junctions_true": 0, "junction_error": 0.0,
                     "ends_pred": 0, "ends_true": 0, "isolated_pred": 0, "isolated_true": 0}
    assert "comparison is the figure" in hostio.graph_metrics.__doc__
    for bad in (np.zeros((2, 63), np.int64), np.zeros((2, 64), np.float64), np.zeros(128, np.int64)):
        with pytest.raises(ValueError, match="jn_hist"):
            hostio.graph_metrics(bad, [1, 1, 0, 1], counts, 1)
    for bad in (np.zeros(3, np.int64), np.zeros(4, np.float64), np.array([1, -1, 1, 1]), 5):
        with pytest.raises(ValueError, match="jn_counts"):
            hostio.graph_metrics(h, bad, counts, 1)
    for bad in (np.zeros(4, np.int64), np.zeros(8, np.float64), -np.ones(8, np.int64)):
        with pytest.raises(ValueError, match="counts"):
            hostio.graph_metrics(h, [1, 1, 0, 1], bad, 1)
    for bad in (-1, 63, 1.0, True, None, "1"):
        with pytest.raises(ValueError, match="slack"):
            hostio.graph_metrics(h, [1, 1, 0, 1], counts, bad)


# ------------------------------------------------------------------------------------------- the bank is not trivial
@pytest.mark.parametrize("kind", ["smooth1.5", "smooth3", "rand0.45"])
def test_pruning_the_thinned_bank_is_not_trivial(kind):
    for shape in ((2, 64, 64), (2, 230, 97)):
        skel = GU.thinned(kind, shape)
        b = hostio.prune_mask(skel, 8)
        ends, iso, junc = hostio.skeleton_nodes(b)
        assert 0 < b.sum() < skel.sum() and ends.any() and junc.any(), (kind, shape)
        assert hostio.skeleton_nodes(skel)[0].sum() > ends.sum()           # the spur tips are gone
    if kind == "smooth1.5":
        skel = GU.thinned(kind, (2, 64, 64))
        b = hostio.prune_mask(skel, 8)
        assert (int(skel.sum()), int(b.sum()), int(hostio.skeleton_nodes(b)[2].sum())) == (949, 702, 44)
