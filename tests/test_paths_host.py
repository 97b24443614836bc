"""No GPU: the eleventh public header include/rsu_paths.h (ordered polylines). The library exports what the header declares and
_lib.SIGNATURES_PATHS binds exactly that, disjoint from the other ten tables; the size function against its stated layout; every refusal
with pointers nobody may follow, the argument error before the size, the 2-GiB refusal one image past the limit; every pointer refused one
step below its alignment and taken at it; the constants of tests/paths_util.py pinned to csrc/paths.hip; the properties of the
restatement hostio.segment_paths on the thinned bank and on the hand masks; simplify_path; road_graph with and without paths; the flags."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from road_segmentation_unet_amd import _lib, hostio
from road_segmentation_unet_amd import model as M
from road_segmentation_unet_amd.cli import parse_options
from tests import align_util as au
from tests import paths_util as PU
from tests import segments_util as SU
from tests import thin_util as TU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["rsu_paths_ws_bytes", "rsu_segment_paths"]
EINVAL = -22
p = ctypes.c_void_p(0x1000)   # a pointer no refused call may follow
OK = (2, 5, 7)


def _header_text():
    return open(os.path.join(ROOT, "include", "rsu_paths.h")).read()


def _protos():
    """{entry: (return type, [(type, name), ...])} of the header, by the parsing of tests/align_util.prototypes"""
    text = re.sub(r"/\*.*?\*/", " ", _header_text(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"^(int|size_t) (rsu_\w+)\(([^;]*?)\);", text, flags=re.M | re.S):
        params = []
        for a in args.split(","):
            m = re.match(r"^(.*?)(\w+)$", " ".join(a.split()))
            params.append((m.group(1).strip(), m.group(2)))
        out[name] = (ret, params)
    return out


def _args(**kw):
    """the arguments of rsu_segment_paths, every pointer the one nobody may follow, sizes that are admitted; kw replaces by name"""
    a = dict(seg=p, edges=p, counts=p, side=0, max_edges=8, max_len=64, max_points=35, paths=p, offsets=p, kind=p, pos=p, info=p, ws=p,
             N=OK[0], H=OK[1], W=OK[2], stream=None)
    assert set(kw) <= set(a), kw
    a.update(kw)
    assert list(a) == [n for _, n in _protos()["rsu_segment_paths"][1]]
    return list(a.values())


# ------------------------------------------------------------------------------------------- ABI
def test_library_exports_the_eleventh_header_and_the_table_binds_it():
    L = _lib.lib()
    protos = _protos()
    assert sorted(protos) == ENTRIES == sorted(_lib.SIGNATURES_PATHS), "ctypes table and rsu_paths.h out of sync"
    for s in ENTRIES:
        assert hasattr(L, s), "librsu_hip.so does not export %s" % s
        assert getattr(L, s).argtypes == _lib.SIGNATURES_PATHS[s][1] and getattr(L, s).restype is _lib.SIGNATURES_PATHS[s][0]
    others = [getattr(_lib, n) for n in dir(_lib) if n.startswith("SIGNATURES") and n != "SIGNATURES_PATHS"]
    assert len(others) == 10
    for t in others:
        assert not set(t) & set(_lib.SIGNATURES_PATHS)
    assert "rsu_paths.h" not in au.HEADERS and not set(ENTRIES) & set(au.prototypes())      # a header of its own: the ten keep their entries
    for ret, (name, (r, params)) in zip(("size_t", "int"), sorted(protos.items())):
        assert r == ret
        kinds = ["i" if t == "int" else "p" for t, _ in params]
        assert all(k == "i" or "*" in t or t == "rsu_stream_t" for k, (t, _) in zip(kinds, params)), name
        assert kinds == ["i" if t is _lib._i else "p" for t in _lib.SIGNATURES_PATHS[name][1]], name
        assert _lib.SIGNATURES_PATHS[name][0] is (_lib._sz if r == "size_t" else _lib._i)
    full = _header_text()
    for macro, value in (("RSU_PATHS_MAX_SIDE", "1024"), ("RSU_PATHS_MAX_EDGES", "65536"), ("RSU_PATHS_MAX_LEN", r"\(1 << 20\)")):
        assert re.search(r"^#define %s %s$" % (macro, value), full, flags=re.M), macro
    assert (_lib.PATHS_MAX_SIDE, _lib.PATHS_MAX_EDGES, _lib.PATHS_MAX_LEN) == (1024, 65536, 1 << 20) \
        == (hostio.PATHS_MAX_SIDE, hostio.PATHS_MAX_EDGES, hostio.PATHS_MAX_LEN) == (PU.MAX_SIDE, PU.MAX_EDGES, PU.MAX_LEN_LIMIT)
    for text in ('#include "rsu.h"', "5 + R", "R = ceil(log2(max_len))", "one arc buffer, 16 N H W bytes", "127 images, and 128 is refused",
                 "An argument error is reported before the size", "need not be cleared and holds nothing between calls", "no scratch",
                 "is range-checked before it addresses", "align (rsu_segment_paths): seg 4, edges 4, counts 4, paths 4, offsets 4, kind 4, pos 4, "
                 "info 4, ws 8. */"):
        assert text in full, text
    for k in ("init", "classify", "rows", "arcs", "jump", "emit"):      # VGPRs, LDS and waves per SIMD of every kernel
        assert re.search(r"k_paths_%s +\d+ VGPRs, +\d+ bytes of LDS, \d waves per SIMD" % k, full), k
    # the tenth header still says what it left out
    assert "Out of scope: ordered polylines" in open(os.path.join(ROOT, "include", "rsu_segments.h")).read()


def test_constants_and_build_are_those_of_the_kernels():
    csrc = os.path.join(ROOT, "road_segmentation_unet_amd", "csrc")
    src = open(os.path.join(csrc, "paths.hip")).read()
    for name, v in (("PT_BLOCK", PU.BLOCK), ("PT_TW", PU.TILE_W), ("PT_TH", PU.TILE_H)):
        assert re.search(r"^#define %s %d\b" % (name, v), src, flags=re.M), name
    assert (hostio.PATHS_BLOCK, hostio.PATHS_TILE) == (PU.BLOCK, (PU.TILE_W, PU.TILE_H)) and hostio._PATH_DIRS == PU.DIRS
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "$(B)/paths.o: HIPFLAGS += -ffp-contract=off" in mk and "$(B)/paths.o " in mk and "../../include/rsu_paths.h" in mk
    code = re.sub(r"//.*", "", src)
    assert not re.search(r"\b(float|double|__threadfence|atomicCAS|atomicExch)\b", code)      # integer only, no flag between workgroups
    assert [PU.rounds(n) for n in (1, 2, 3, 4, 64, 65, 4096, 1 << 20)] == [0, 1, 2, 2, 6, 7, 12, 20] \
        == [hostio.path_rounds(n) for n in (1, 2, 3, 4, 64, 65, 4096, 1 << 20)]


def test_size_function_against_its_layout_and_the_refusals():
    L = _lib.lib()
    for shape in SU.SHAPES + [(4, 388, 388), (2, 608, 608), (1, 1024, 1024), (127, 1024, 1024)]:
        for cap in (1, 4096, 65536):
            for max_len in (1, 2, 64, 65, 4096, 1 << 20):
                need = L.rsu_paths_ws_bytes(*shape, cap, max_len)
                assert need == PU.ws_layout(*shape, cap, max_len) and need % 8 == 0 and need > 0, (shape, cap, max_len)
    bad_sizes = ((0, 5, 5), (5, 0, 5), (5, 5, 0), (-1, 5, 5), (5, -1, 5), (5, 5, -1), (1, 1025, 5), (1, 5, 1025), (1, 1 << 20, 1))
    for bad in bad_sizes + ((128, 1024, 1024), (1 << 30, 2, 1)):
        assert L.rsu_paths_ws_bytes(*bad, 8, 64) == 0, bad
    bad_caps, bad_lens = (0, -1, 65537, 1 << 30, -(1 << 31)), (0, -1, (1 << 20) + 1, 1 << 30, -(1 << 31))
    for cap in bad_caps:
        assert L.rsu_paths_ws_bytes(*OK, cap, 64) == 0, cap
    for n in bad_lens:
        assert L.rsu_paths_ws_bytes(*OK, 8, n) == 0, n
    G = L.rsu_segment_paths
    for name in ("seg", "edges", "counts", "paths", "offsets", "kind", "info", "ws"):
        assert G(*_args(**{name: None})) == EINVAL, name
    for bad in bad_sizes:
        assert G(*_args(N=bad[0], H=bad[1], W=bad[2], max_points=1)) == EINVAL, bad
    for side in (-1, 2, 1 << 30):
        assert G(*_args(side=side)) == EINVAL, side
    for cap in bad_caps:
        assert G(*_args(max_edges=cap)) == EINVAL, cap
    for n in bad_lens:
        assert G(*_args(max_len=n)) == EINVAL, n
    for n in (0, -1, 36, 1 << 30):      # max_points outside [1, H W]
        assert G(*_args(max_points=n)) == EINVAL, n


def test_two_gib_refusal_one_image_past_the_limit():
    L = _lib.lib()
    S = 1024
    assert 127 * S * S * 16 < 0x7ffffff0 <= 128 * S * S * 16
    assert L.rsu_paths_ws_bytes(127, S, S, 4096, 4096) == PU.ws_layout(127, S, S, 4096, 4096) > 0 and L.rsu_paths_ws_bytes(128, S, S, 4096, 4096) == 0
    G = L.rsu_segment_paths
    big = dict(N=128, H=S, W=S, max_points=S * S)
    assert G(*_args(**big)) == _lib.E2BIG and G(*_args(pos=None, **big)) == _lib.E2BIG and G(*_args(**dict(big, N=255))) == _lib.E2BIG
    with pytest.raises(_lib.RsuError, match="2 GiB"):
        _lib.call("rsu_segment_paths", *_args(**big))
    # a wrong argument is reported before the size
    for kw in (dict(seg=None), dict(side=2), dict(max_edges=0), dict(max_len=0), dict(ws=None), dict(ws=ctypes.c_void_p(0x1004)),
               dict(info=ctypes.c_void_p(0x1002))):
        assert G(*_args(**dict(big, **kw))) == EINVAL, kw
    assert G(*_args(**dict(big, max_points=S * S + 1))) == EINVAL


def test_every_pointer_is_refused_below_its_alignment_and_taken_at_it():
    """the size of a refused batch makes an admitted pointer visible without a launch: RSU_E2BIG is returned behind the alignment check"""
    L = _lib.lib()
    G = L.rsu_segment_paths
    notes = re.findall(r"align \(rsu_segment_paths\): (.*?)\. \*/", _header_text())
    assert len(notes) == 1
    align = {k: int(v) for k, v in (item.split() for item in notes[0].split(", "))}
    pointers = [n for t, n in _protos()["rsu_segment_paths"][1] if "*" in t]
    assert sorted(align) == sorted(pointers) and align == dict({n: 4 for n in pointers}, ws=8)
    big = dict(N=128, H=1024, W=1024, max_points=1)
    for name, a in align.items():
        base = 0x10000
        assert G(*_args(**dict(big, **{name: ctypes.c_void_p(base + a)}))) == _lib.E2BIG, name          # at its number: taken
        for step in (a // 2, 1, a + a // 2):
            assert G(*_args(**dict(big, **{name: ctypes.c_void_p(base + step)}))) == EINVAL, (name, step)
            assert G(*_args(**{name: ctypes.c_void_p(base + step)})) == EINVAL, (name, step)            # and at an admitted size


def test_the_fenced_file_launches_the_entry_with_an_exact_workspace():
    from tests import test_gpu_paths_fenced as G
    assert sorted(G.FENCED) == ["rsu_segment_paths"]
    tests = {n: f for n, f in vars(G).items() if n.startswith("test_") and callable(f)}
    for n in G.FENCED["rsu_segment_paths"]:
        assert n in tests and '"rsu_segment_paths"' in inspect.getsource(tests[n]) + "".join(inspect.getsource(h) for h in G.HELPERS.get(n, ()))
    assert "pytest.mark.gpu" in inspect.getsource(G) and "rsu_paths_ws_bytes" in inspect.getsource(G)


# ------------------------------------------------------------------------------------------- the restatement
def _properties(seg, edges, counts, side, out, max_len, what):
    """what include/rsu_paths.h promises of (paths, offsets, kind, pos, info), checked with links formed apart from hostio's"""
    paths, offsets, kind, pos, info = out
    N, H, W = seg.shape
    cap = edges.shape[1]
    seen = np.zeros(4, np.int64)
    for n in range(N):
        stored = min(int(counts[n, 2 * side]), cap)
        links = PU.link_mask(seg[n] != 0)
        degree = np.zeros(H * W, np.int64)
        for a, b in (tuple(l) for l in links):
            degree[a] += 1
            degree[b] += 1
        assert (kind[n, stored:] == PU.FILL).all() and (offsets[n, stored + 1:] == PU.FILL).all(), (what, n)
        total, ordered = 0, np.zeros((H, W), np.int32)
        for r in range(stored):
            label, pixels = int(edges[n, r, 0]), int(edges[n, r, 1])
            own = np.nonzero(seg[n].reshape(-1) == label)[0]
            assert own.size == pixels and own[0] == label - 1, (what, n, r)
            k = int(kind[n, r])
            want = PU.LONG if pixels > max_len else PU.BRANCHED if (degree[own] >= 3).any() else PU.OPEN if (degree[own] <= 1).any() else PU.RING
            assert k == want and int(offsets[n, r]) == total, (what, n, r, k, want)
            seen[k] += 1
            if k > 1:
                continue
            pts = paths[n, total:total + pixels]
            total += pixels
            assert sorted(pts.tolist()) == own.tolist(), (what, n, r, "not a permutation of the segment's pixels")
            assert all(frozenset((int(a), int(b))) in links for a, b in zip(pts[:-1], pts[1:])), (what, n, r, "a step that is no link")
            ends = own[degree[own] <= 1]
            if k == PU.OPEN:
                assert ends.size == (2 if pixels > 1 else 1) and pts[0] == ends.min() and pts[-1] == ends.max(), (what, n, r)
            else:
                nb = sorted(int(next(iter(l - {label - 1}))) for l in links if label - 1 in l)
                assert pts[0] == label - 1 and len(nb) == 2 and pts[1] == nb[0] and pts[-1] == nb[1], (what, n, r)
                assert frozenset((int(pts[-1]), int(pts[0]))) in links
            ordered.reshape(-1)[pts] = 1 + np.arange(pixels)
        assert np.array_equal(pos[n], ordered), (what, n)
        assert int(offsets[n, stored]) == total and (paths[n, total:] == PU.FILL).all(), (what, n)
        k = kind[n, :stored]
        assert info[n].tolist() == [total, int((k == 0).sum()), int((k == 1).sum()), int((k >= 2).sum())], (what, n)
    return seen


@pytest.mark.parametrize("L", SU.PRUNES)
@pytest.mark.parametrize("shape", PU.HOST_SHAPES, ids=SU.shape_id)
def test_restatement_on_the_thinned_bank(shape, L):
    seen = np.zeros(4, np.int64)
    for name in TU.pair_names():
        for side in (0, 1):
            seg, edges, counts = PU.bank_inputs(name, shape, L, side)
            out = PU.bank_host(name, shape, L, side)
            seen += _properties(seg, edges, counts, side, out, PU.MAX_LEN, (name, shape, L, side))
    assert seen[PU.OPEN] > 100 and seen[PU.BRANCHED] > 0 and seen[PU.LONG] == 0 and (seen[PU.RING] > 0 or shape[1] < 100), seen


def test_restatement_on_the_hand_masks():
    cases = PU.hand_cases()
    small = PU.inputs_of(cases["small"])
    out = PU.host(*small, 0, 64, 12 * 16)
    _properties(*small, 0, out, 64, "small")
    assert out[2][:, 0].tolist() == [PU.OPEN] * 4 + [PU.RING] * 2 + [PU.BRANCHED] and small[2][:, 0].tolist() == [1] * 7
    assert out[4].tolist() == [[1, 1, 0, 0], [2, 1, 0, 0], [8, 1, 0, 0], [16, 1, 0, 0], [4, 0, 1, 0], [4, 0, 1, 0], [0, 0, 0, 1]]
    W = 16
    assert out[0][4, :4].tolist() == [4 * W + 6, 4 * W + 7, 5 * W + 7, 5 * W + 6]      # the block: from its first pixel clockwise
    assert out[0][5, :4].tolist() == [4 * W + 7, 5 * W + 6, 6 * W + 7, 5 * W + 8]      # the diamond: towards the smaller neighbour
    assert out[0][2, :8].tolist() == [3 * W + 4, 4 * W + 4, 5 * W + 4, 6 * W + 4, 6 * W + 5, 6 * W + 6, 6 * W + 7, 6 * W + 8]      # the L
    for name in ("diagonal", "stairs", "rings", "two_images"):
        inp = PU.inputs_of(cases[name])
        hw = cases[name].shape[1] * cases[name].shape[2]
        out = PU.host(*inp, 0, 4096, hw)
        seen = _properties(*inp, 0, out, 4096, name)
        assert seen.tolist() == {"diagonal": [1, 0, 0, 0], "stairs": [1, 0, 0, 0], "rings": [0, 2, 0, 0], "two_images": [2, 0, 0, 0]}[name], (name, seen)
    rings = PU.host(*PU.inputs_of(cases["rings"]), 0, 4096, 24 * 96)
    assert rings[0][0, [0, 12]].tolist() == [PU.BLOCK - 1, 4 * PU.BLOCK] and rings[0][0, [1, 13]].tolist() == [PU.BLOCK, 4 * PU.BLOCK + 1]
    for (max_len, n), mask in PU.serpentine_cases().items():
        inp = PU.inputs_of(mask)
        out = PU.host(*inp, 0, max_len, 64 * 64)
        assert inp[2][0, 0] == 1 and inp[1][0, 0, 1] == n and out[2][0, 0] == (PU.OPEN if n <= max_len else PU.LONG), (max_len, n)
        assert out[4][0].tolist() == ([n, 1, 0, 0] if n <= max_len else [0, 0, 0, 1])
        _properties(*inp, 0, out, max_len, ("serpentine", max_len, n))
    u = PU.inputs_of(PU.uneven())
    assert u[1][0, 0, 1] == 1400 and u[2][:, 0].tolist() == [1, 3, 0] and PU.rounds(1400 - 1) == 11
    _properties(*u, 0, PU.host(*u, 0, 4096, 40 * 300), 4096, "uneven")


def test_truncation_side_and_fill_of_the_restatement():
    shape, name = (2, 230, 97), "smooth1.5~smooth3"
    seg, edges, counts = PU.bank_inputs(name, shape, 8, 1)
    full = PU.bank_host(name, shape, 8, 1)
    total = int(full[4][:, 0].max())
    assert total > 400 and int(counts[:, 2].min()) > 20
    cut = PU.host(seg, edges, counts, 1, PU.MAX_LEN, total // 2)      # max_points below the total: the head is the same, info the true number
    assert np.array_equal(cut[0], full[0][:, :total // 2]) and all(np.array_equal(a, b) for a, b in zip(cut[1:], full[1:]))
    few = PU.host(seg, edges[:, :5].copy(), counts, 1, PU.MAX_LEN, shape[1] * shape[2])      # max_edges below the count: rows dropped
    assert np.array_equal(few[2], full[2][:, :5]) and np.array_equal(few[1][:, :6], full[1][:, :6])
    assert ((few[3] > 0) <= (full[3] > 0)).all() and (few[3] > 0).sum() < (full[3] > 0).sum()
    short = PU.host(seg, edges, counts, 1, 10, shape[1] * shape[2])
    assert ((short[2] == PU.LONG) == ((edges[:, :, 1] > 10) & (short[2] != PU.FILL))).all() and (short[2] == PU.LONG).any()
    other = hostio.segment_paths(seg, edges, counts, 1, PU.MAX_LEN, shape[1] * shape[2], fill=5)
    assert (other[2][full[2] == PU.FILL] == 5).all() and (other[0][full[0] == PU.FILL] == 5).all()


def test_restatement_rejects_what_the_header_rejects():
    seg, edges, counts = PU.inputs_of(PU.hand_cases()["small"])
    hw = 12 * 16
    hostio.segment_paths(seg, edges, counts, 0, 1, 1)
    hostio.segment_paths(seg, edges, counts, 1, 1 << 20, hw)
    for kw in (dict(side=2), dict(side=-1), dict(side=True), dict(max_len=0), dict(max_len=(1 << 20) + 1), dict(max_len=2.0), dict(max_points=0),
               dict(max_points=hw + 1), dict(seg=seg[0]), dict(seg=seg.astype(np.float32)), dict(edges=edges[:, :, :7]), dict(edges=edges[:3]),
               dict(counts=counts[:, :3]), dict(seg=np.zeros((1, 1025, 2), np.int32), edges=edges[:1], counts=counts[:1])):
        a = dict(seg=seg, edges=edges, counts=counts, side=0, max_len=64, max_points=hw)
        a.update(kw)
        with pytest.raises(ValueError, match="segment_paths"):
            hostio.segment_paths(**a)


# ------------------------------------------------------------------------------------------- simplify_path, road_graph
def test_simplify_path():
    line = np.stack([np.arange(20), 3 + 2 * np.arange(20)], axis=1)
    assert hostio.simplify_path(line, 0.5).tolist() == [[0, 3], [19, 41]]
    ell = np.array([[y, 4] for y in range(3, 7)] + [[6, x] for x in range(5, 9)])
    assert hostio.simplify_path(ell, 0.5).tolist() == [[3, 4], [6, 4], [6, 8]]
    assert hostio.simplify_path(ell, 100.0).tolist() == [[3, 4], [6, 8]]      # the first and the last point stay
    wiggle = np.array([[0, 0], [1, 1], [0, 2], [1, 3], [0, 4]])
    assert hostio.simplify_path(wiggle, 1.5).tolist() == [[0, 0], [0, 4]] and hostio.simplify_path(wiggle, 0.5).tolist() == wiggle.tolist()
    assert hostio.simplify_path(wiggle, 0.9).tolist() == [[0, 0], [1, 1], [0, 4]]      # (0, 2) and (1, 3) lie 2 / sqrt(10) from (1, 1) - (0, 4)
    for pts in (line, ell, wiggle, line[:1], line[:2], line[:0]):
        out = hostio.simplify_path(pts, 0)
        assert out.tolist() == pts.tolist() and out.dtype == pts.dtype and out is not pts      # eps = 0: the identity
    ring = np.array([[0, 0], [0, 1], [0, 2], [1, 2], [2, 2], [2, 1], [2, 0], [1, 0]])      # cut at its first point: an open chain to its last pixel
    assert hostio.simplify_path(ring, 0.5).tolist() == [[0, 0], [0, 2], [2, 2], [2, 0], [1, 0]]
    for bad, eps in ((line.astype(np.float32), 1), (line.reshape(-1), 1), (line, -1), (line, float("nan")), (line, "1"), (line, True)):
        with pytest.raises(ValueError, match="simplify_path"):
            hostio.simplify_path(bad, eps)


def _parent_road_graph(edges, count, node_map, H, W):
    """road_graph as it was before it took paths: the dict of today, key for key"""
    rows = np.asarray(edges)[:min(int(count), len(edges))].astype(np.int64)
    lone = set(int(-r[4]) for r in rows if r[1] == 1 and r[6] == 0 and r[7] == 1)
    nodes = []
    ys, xs = np.nonzero(node_map)
    ids = node_map[ys, xs].astype(np.int64)
    for i in np.unique(ids):
        sel = ids == i
        nodes.append({"id": int(i), "kind": "junction", "y": float(ys[sel].mean()), "x": float(xs[sel].mean())} if i > 0 else
                     {"id": int(i), "kind": "isolated" if int(-i) in lone else "end", "y": float(ys[sel][0]), "x": float(xs[sel][0])})
    root2 = float(np.sqrt(np.float64(2.0)))
    return {"nodes": nodes, "edges": [{"id": int(r[0]), "a": int(r[4]), "b": int(r[5]), "pixels": int(r[1]),
                                       "length": float(r[2]) + root2 * float(r[3]), "contacts": int(r[6]), "ends": int(r[7])} for r in rows]}


def test_road_graph_with_and_without_paths():
    shape, name = (2, 230, 97), "smooth1.5~smooth3"
    H, W = shape[1:]
    ref = SU.host_pair(name, shape, 8)
    out = PU.bank_host(name, shape, 8, 0)
    reversed_, kinds = 0, set()
    for n in range(shape[0]):
        plain = hostio.road_graph(ref[0][n], int(ref[2][n, 0]), ref[5][n], H, W)
        assert plain == _parent_road_graph(ref[0][n], int(ref[2][n, 0]), ref[5][n], H, W) == hostio.road_graph(ref[0][n], int(ref[2][n, 0]), ref[5][n], H, W, paths=None)
        assert [list(e) for e in plain["edges"]][:1] == [["id", "a", "b", "pixels", "length", "contacts", "ends"]]
        g = hostio.road_graph(ref[0][n], int(ref[2][n, 0]), ref[5][n], H, W, paths=(out[0][n], out[1][n], out[2][n]))
        assert g["nodes"] == plain["nodes"] and len(g["edges"]) == len(plain["edges"]) > 20
        for r, (e, q) in enumerate(zip(g["edges"], plain["edges"])):
            assert {k: v for k, v in e.items() if k not in ("kind", "path")} == q and list(e)[-2:] == ["kind", "path"]
            k = int(out[2][n, r])
            assert e["kind"] == ("open", "ring", "branched", "long")[k]
            kinds.add(e["kind"])
            device = [[int(v) // W, int(v) % W] for v in out[0][n, out[1][n, r]:out[1][n, r] + e["pixels"]]] if k <= 1 else []
            assert e["path"] in (device, device[::-1])
            if e["path"] != device:
                reversed_ += 1
            if k == 0 and e["pixels"] > 1 and e["a"] != e["b"]:      # from a to b wherever only one end touches a
                first, last = (hostio._node_touches(ref[5][n], e["a"], *e["path"][i]) for i in (0, -1))
                assert first or not last, (n, r)
    assert reversed_ > 0 and {"open"} <= kinds
    with pytest.raises(ValueError, match="road_graph"):
        hostio.road_graph(ref[0][0], int(ref[2][0, 0]), ref[5][0], H, W, paths=(out[0][0], out[1][0][:-1], out[2][0]))
    # a hand case: an end at the LAST pixel of the device order (its index is the larger one) and a junction zone at the first
    m = np.zeros((1, 20, 20), bool)
    m[0, 3, 2:15] = m[0, 3:12, 8] = True      # a T: three branches from one zone
    ref = hostio.line_segments(m.astype(np.float32), 0.5, None, 16)
    seg, edges, counts = ref[3], ref[0], ref[2]
    out = hostio.segment_paths(seg, edges, counts, 0, 64, 400)
    g = hostio.road_graph(edges[0], int(counts[0, 0]), ref[5][0], 20, 20, paths=(out[0][0], out[1][0], out[2][0]))
    assert len(g["edges"]) == 3
    for e in g["edges"]:
        assert e["kind"] == "open" and e["a"] < 0 < e["b"] and ref[5][0][tuple(e["path"][0])] == e["a"], e      # every branch runs from its end


def test_the_flags_and_their_refusals():
    defs = {d[0]: d for d in M.EXTRA_FLAG_DEFS}
    assert defs["road_graph_paths"][1:3] == (bool, False) and defs["max_path_length"][1:3] == (int, 4096) and defs["road_graph_simplify"][1:3] == (float, 0.0)
    for o in (M.Options(), parse_options([])):
        assert (o.road_graph_paths, o.max_path_length, o.road_graph_simplify) == (False, 4096, 0.0)
    o = parse_options(["--save_road_graph", "--road_graph_paths", "--max_path_length=1048576", "--road_graph_simplify=1.5"])
    assert (o.save_road_graph, o.road_graph_paths, o.max_path_length, o.road_graph_simplify) == (True, True, 1 << 20, 1.5)
    assert M.parse_max_path_length("7") == 7 and isinstance(M.parse_max_path_length(np.int64(3)), int) and M.parse_road_graph_simplify("0") == 0.0
    for bad in (0, -1, (1 << 20) + 1, 2.5, True, None, "x"):
        with pytest.raises(ValueError, match="max_path_length"):
            M.parse_max_path_length(bad)
        with pytest.raises(ValueError, match="max_path_length"):
            M.Options(max_path_length=bad)
    for bad in (-0.5, float("nan"), float("inf"), True, None, "x"):
        with pytest.raises(ValueError, match="road_graph_simplify"):
            M.parse_road_graph_simplify(bad)
        with pytest.raises(ValueError, match="road_graph_simplify"):
            M.Options(road_graph_simplify=bad)
    from road_segmentation_unet_amd import mask_metrics
    assert mask_metrics._WS["paths"][0] == "rsu_paths_ws_bytes"
