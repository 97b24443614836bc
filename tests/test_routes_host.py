"""No GPU: the twelfth public header include/rsu_routes.h (network distances and the path-length score). The library exports what the
header declares and _lib.ROUTES_SIGNATURES binds exactly that, disjoint from the other eleven tables; the size function against its
stated layout; every refusal with pointers nobody may follow, the argument error before the size, the 2-GiB refusals one image past the
limit; every pointer refused one step below its alignment and taken at it; the restatement hostio.graph_routes against scipy's shortest
paths on the thinned bank and on hand graphs, its symmetry and the triangle inequality; hostio.route_score on cases worked out by hand;
route_metrics; the flags and the accumulator's new stage."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from road_segmentation_unet_amd import _lib, hostio
from road_segmentation_unet_amd import mask_metrics as MM
from road_segmentation_unet_amd import model as M
from road_segmentation_unet_amd.cli import parse_options
from tests import routes_util as RU
from tests import segments_util as SU

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["rsu_graph_routes", "rsu_route_score", "rsu_routes_ws_bytes"]
EINVAL = -22
p = ctypes.c_void_p(0x1000)   # a pointer no refused call may follow
OK = (2, 5, 7)
INF, Q = RU.INF, RU.Q


def _header_text():
    return open(os.path.join(ROOT, "include", "rsu_routes.h")).read()


def _protos():
    """{entry: (return type, [(type, name), ...])} of the header"""
    text = re.sub(r"/\*.*?\*/", " ", _header_text(), flags=re.S)
    out = {}
    for ret, name, args in re.findall(r"^(int|size_t) (rsu_\w+)\(([^;]*?)\);", text, flags=re.M | re.S):
        params = []
        for a in args.split(","):
            m = re.match(r"^(.*?)(\w+)$", " ".join(a.split()))
            params.append((m.group(1).strip(), m.group(2)))
        out[name] = (ret, params)
    return out


def _routes_args(**kw):
    """the arguments of rsu_graph_routes, every pointer the one nobody may follow, sizes that are admitted; kw replaces by name"""
    a = dict(node_map=p, edges=p, counts=p, side=0, max_edges=8, max_nodes=16, nodes=p, dist=p, info=p, ws=p, N=OK[0], H=OK[1], W=OK[2],
             stream=None)
    assert set(kw) <= set(a), kw
    a.update(kw)
    assert list(a) == [n for _, n in _protos()["rsu_graph_routes"][1]]
    return list(a.values())


def _score_args(**kw):
    a = dict(nodes_a=p, dist_a=p, info_a=p, nodes_b=p, dist_b=p, info_b=p, max_nodes=16, slack=8, match=p, acc=p, N=2, stream=None)
    assert set(kw) <= set(a), kw
    a.update(kw)
    assert list(a) == [n for _, n in _protos()["rsu_route_score"][1]]
    return list(a.values())


ARGS = {"rsu_graph_routes": _routes_args, "rsu_route_score": _score_args}
BIG = {"rsu_graph_routes": dict(N=512, H=1024, W=1024), "rsu_route_score": dict(N=512, max_nodes=1024)}      # refused for their size alone


# ------------------------------------------------------------------------------------------- ABI
def test_library_exports_the_twelfth_header_and_the_table_binds_it():
    L = _lib.lib()
    protos = _protos()
    assert sorted(protos) == ENTRIES == sorted(_lib.ROUTES_SIGNATURES), "ctypes table and rsu_routes.h out of sync"
    for s in ENTRIES:
        assert hasattr(L, s), "librsu_hip.so does not export %s" % s
        assert getattr(L, s).argtypes == _lib.ROUTES_SIGNATURES[s][1] and getattr(L, s).restype is _lib.ROUTES_SIGNATURES[s][0]
    others = [getattr(_lib, n) for n in dir(_lib) if n.startswith("SIGNATURES")]      # (the eleven earlier tables share that prefix)
    assert len(others) == 11 and [n for n in dir(_lib) if n.endswith("_SIGNATURES")] == ["ROUTES_SIGNATURES"]
    for t in others:
        assert not set(t) & set(_lib.ROUTES_SIGNATURES)
    for name, (r, params) in protos.items():
        kinds = ["i" if t == "int" else "p" for t, _ in params]
        assert all(k == "i" or "*" in t or t == "rsu_stream_t" for k, (t, _) in zip(kinds, params)), name
        assert kinds == ["i" if t is _lib._i else "p" for t in _lib.ROUTES_SIGNATURES[name][1]], name
        assert _lib.ROUTES_SIGNATURES[name][0] is (_lib._sz if r == "size_t" else _lib._i)
    full = _header_text()
    for macro, value in (("RSU_ROUTES_MAX_SIDE", "1024"), ("RSU_ROUTES_MAX_NODES", "1024"), ("RSU_ROUTES_INF", "0x3fffffff"), ("RSU_ROUTES_Q", "65536")):
        assert re.search(r"^#define %s %s$" % (macro, value), full, flags=re.M), macro
    assert (_lib.ROUTES_MAX_SIDE, _lib.ROUTES_MAX_NODES, _lib.ROUTES_INF, _lib.ROUTES_Q) == (1024, 1024, INF, Q) \
        == (hostio.ROUTES_MAX_SIDE, hostio.ROUTES_MAX_NODES, hostio.ROUTES_INF, hostio.ROUTES_Q) == (RU.MAX_SIDE, RU.MAX_NODES, RU.INF, RU.Q)
    for text in ('#include "rsu.h"', "8 + 2 T", "T = ceil(max_nodes / 64)", "511 images, and 512 is refused", "sum(y) <= 1023 * 2^20",
                 "An argument error is reported before the size", "need not be cleared and holds nothing between calls", "no scratch",
                 "is range-checked before it addresses", "points injected along edges", "skips the interiors of", "Everything is per image",
                 "align (rsu_graph_routes): node_map 4, edges 4, counts 4, nodes 4, dist 4, info 4, ws 4. */",
                 "align (rsu_route_score): nodes_a 4, dist_a 4, info_a 4, nodes_b 4, dist_b 4, info_b 4, match 4, acc 8. */"):
        assert text in full, text
    for k in ("count", "scan", "place", "fill", "sums", "close", "edges", "diag", "cross", "rest", "match", "pairs"):
        assert re.search(r"k_routes_%s +\d+ VGPRs, +\d+ bytes of LDS, \d waves per SIMD" % k, full), k      # of every kernel


def test_constants_and_build_are_those_of_the_kernels():
    csrc = os.path.join(ROOT, "road_segmentation_unet_amd", "csrc")
    src = open(os.path.join(csrc, "routes.hip")).read()
    for name, v in (("RT_BLOCK", RU.BLOCK), ("RT_TILE", RU.TILE)):
        assert re.search(r"^#define %s %d\b" % (name, v), src, flags=re.M), name
    assert (hostio.ROUTES_BLOCK, hostio.ROUTES_TILE) == (RU.BLOCK, RU.TILE) and (hostio.ROUTES_ORTHO, hostio.ROUTES_DIAG) == (70, 99)
    assert abs(99.0 / 70.0 / np.sqrt(2.0) - 1.0) < 1e-4 and 99 * (1 << 20) < INF and 2 * INF < (1 << 31)
    mk = open(os.path.join(csrc, "Makefile")).read()
    assert "$(B)/routes.o: HIPFLAGS += -ffp-contract=off" in mk and "$(B)/routes.o " in mk and "../../include/rsu_routes.h" in mk
    code = re.sub(r"//.*", "", src)
    assert not re.search(r"\b(float|double|__threadfence|atomicCAS|atomicExch)\b", code)      # integer only, no flag between workgroups
    assert [RU.rounds(n) for n in (1, 64, 65, 100, 256, 1024)] == [1, 1, 2, 2, 4, 16] and RU.launches(1024) == 40 and RU.launches(64) == 10


def test_size_function_against_its_layout_and_the_refusals():
    L = _lib.lib()
    for shape in SU.SHAPES + [(4, 388, 388), (2, 608, 608), (1, 1024, 1024), (511, 1024, 1024)]:
        for cap in (1, 64, 100, 256, 1024):
            if shape[0] * cap * cap * 4 < 0x7ffffff0:
                need = L.rsu_routes_ws_bytes(*shape, cap)
                assert need == RU.ws_layout(*shape, cap) and need % 4 == 0 and need > 0, (shape, cap)
    bad_sizes = ((0, 5, 5), (5, 0, 5), (5, 5, 0), (-1, 5, 5), (5, -1, 5), (5, 5, -1), (1, 1025, 5), (1, 5, 1025), (1, 1 << 20, 1))
    for bad in bad_sizes + ((512, 1024, 1024), (1 << 30, 2, 1)):
        assert L.rsu_routes_ws_bytes(*bad, 16) == 0, bad
    bad_nodes, bad_caps = (0, -1, 1025, 1 << 30, -(1 << 31)), (0, -1, 65537, 1 << 30, -(1 << 31))
    for cap in bad_nodes:
        assert L.rsu_routes_ws_bytes(*OK, cap) == 0, cap
    assert L.rsu_routes_ws_bytes(511, 32, 32, 1024) == RU.ws_layout(511, 32, 32, 1024) and L.rsu_routes_ws_bytes(512, 32, 32, 1024) == 0
    G, S = L.rsu_graph_routes, L.rsu_route_score
    for name in ("node_map", "edges", "counts", "nodes", "dist", "info", "ws"):
        assert G(*_routes_args(**{name: None})) == EINVAL, name
    for name in ("nodes_a", "dist_a", "info_a", "nodes_b", "dist_b", "info_b", "match", "acc"):
        assert S(*_score_args(**{name: None})) == EINVAL, name
    for bad in bad_sizes:
        assert G(*_routes_args(N=bad[0], H=bad[1], W=bad[2])) == EINVAL, bad
    for side in (-1, 2, 1 << 30):
        assert G(*_routes_args(side=side)) == EINVAL, side
    for cap in bad_caps:
        assert G(*_routes_args(max_edges=cap)) == EINVAL, cap
    for cap in bad_nodes:
        assert G(*_routes_args(max_nodes=cap)) == EINVAL and S(*_score_args(max_nodes=cap)) == EINVAL, cap
    for n in (0, -1, -(1 << 31)):
        assert S(*_score_args(N=n)) == EINVAL, n
    for slack in (-1, 1024, 1 << 30):
        assert S(*_score_args(slack=slack)) == EINVAL, slack


def test_two_gib_refusals_one_image_past_the_limit():
    L = _lib.lib()
    G, S = L.rsu_graph_routes, L.rsu_route_score
    assert 511 * 1024 * 1024 * 4 < 0x7ffffff0 <= 512 * 1024 * 1024 * 4
    for big in (dict(N=512, H=1024, W=1024, max_nodes=64), dict(N=512, H=32, W=32, max_nodes=1024), dict(N=1 << 20, H=1, W=1, max_nodes=1024)):
        assert G(*_routes_args(**big)) == _lib.E2BIG, big
        # a wrong argument is reported before the size
        for kw in (dict(node_map=None), dict(side=2), dict(max_edges=0), dict(ws=None), dict(ws=ctypes.c_void_p(0x1002)), dict(info=ctypes.c_void_p(0x1001))):
            assert G(*_routes_args(**dict(big, **kw))) == EINVAL, kw
    assert S(*_score_args(N=512, max_nodes=1024)) == _lib.E2BIG and S(*_score_args(N=512, max_nodes=1024, slack=-1)) == EINVAL
    assert S(*_score_args(N=512, max_nodes=1024, acc=ctypes.c_void_p(0x1004))) == EINVAL
    with pytest.raises(_lib.RsuError, match="2 GiB"):
        _lib.call("rsu_graph_routes", *_routes_args(N=512, H=1024, W=1024))


@pytest.mark.parametrize("entry", ["rsu_graph_routes", "rsu_route_score"])
def test_every_pointer_is_refused_below_its_alignment_and_taken_at_it(entry):
    """the size of a refused batch makes an admitted pointer visible without a launch: RSU_E2BIG is returned behind the alignment check"""
    G = getattr(_lib.lib(), entry)
    notes = re.findall(r"align \(%s\): (.*?)\. \*/" % entry, _header_text())
    assert len(notes) == 1
    align = {k: int(v) for k, v in (item.split() for item in notes[0].split(", "))}
    pointers = [n for t, n in _protos()[entry][1] if "*" in t]
    assert sorted(align) == sorted(pointers) and align == dict({n: 4 for n in pointers}, **({"acc": 8} if entry == "rsu_route_score" else {}))
    for name, a in align.items():
        base = 0x10000
        assert G(*ARGS[entry](**dict(BIG[entry], **{name: ctypes.c_void_p(base + a)}))) == _lib.E2BIG, name          # at its number: taken
        for step in (a // 2, 1, a + a // 2):
            assert G(*ARGS[entry](**dict(BIG[entry], **{name: ctypes.c_void_p(base + step)}))) == EINVAL, (name, step)
            assert G(*ARGS[entry](**{name: ctypes.c_void_p(base + step)})) == EINVAL, (name, step)                    # and at an admitted size


def test_the_fenced_file_launches_both_entries_with_an_exact_workspace():
    from tests import test_gpu_routes_fenced as G
    assert sorted(G.FENCED) == ["rsu_graph_routes", "rsu_route_score"]
    tests = {n: f for n, f in vars(G).items() if n.startswith("test_") and callable(f)}
    for entry, names in G.FENCED.items():
        for n in names:
            assert n in tests and '"%s"' % entry in inspect.getsource(tests[n]) + "".join(inspect.getsource(h) for h in G.HELPERS.get(n, ()))
    assert "pytest.mark.gpu" in inspect.getsource(G) and "rsu_routes_ws_bytes" in inspect.getsource(G)


# ------------------------------------------------------------------------------------------- the restatement of the distances
def _independent(node_map, edges, count):
    """(ids in ascending |id|, all-pairs lengths by scipy) of one image, formed apart from hostio's code"""
    ids = sorted(set(int(v) for v in node_map.reshape(-1) if v), key=abs)
    row = {v: i for i, v in enumerate(ids)}
    rows = [(row[int(r[4])], row[int(r[5])], int(r[2]), int(r[3])) for r in edges[:count] if r[4] != r[5]]
    return ids, RU.reference_distances(len(ids), rows)


@pytest.mark.parametrize("L", SU.PRUNES)
@pytest.mark.parametrize("shape", RU.SHAPES, ids=SU.shape_id)
def test_restatement_against_scipy_on_the_thinned_bank(shape, L):
    most = 0
    for name in RU.BANK:
        for side in (0, 1):
            node_map, edges, counts = RU.bank_inputs(name, shape, L, side)
            nodes, dist, info = RU.bank_host(name, shape, L, side)
            for n in range(shape[0]):
                ids, ref = _independent(node_map[n], edges[n], int(counts[n, 2 * side]))
                k = len(ids)
                most = max(most, k)
                assert info[n, :2].tolist() == [k, k] and info[n, 3] == 0 and nodes[n, :k, 0].tolist() == ids, (name, side, n)
                assert info[n, 2] == sum(1 for r in edges[n, :counts[n, 2 * side]] if r[4] != r[5])
                D = dist[n, :k, :k].astype(np.int64)
                assert np.array_equal(D, ref), (name, side, n)
                assert np.array_equal(D, D.T) and (np.diag(D) == 0).all() and ((D >= 0) & (D <= INF)).all()      # symmetric
                assert (dist[n, k:] == RU.FILL).all() and (dist[n, :, k:] == RU.FILL).all() and (nodes[n, k:] == RU.FILL).all()
                if 0 < k <= 200:      # the triangle inequality, with sums cut at INF
                    assert (D[:, None, :] <= np.minimum(D[:, :, None] + D[None, :, :], INF)).all(), (name, side, n)
                # positions: an end's pixel, a zone's rounded centroid
                W = shape[2]
                for r in range(0, k, max(k // 25, 1)):
                    i, y, x, px = (int(v) for v in nodes[n, r])
                    if i < 0:
                        assert (y * W + x, px) == (-i - 1, 1)
                    else:
                        ys, xs = np.nonzero(node_map[n] == i)
                        assert px == ys.size and (y, x) == (int(np.floor(ys.mean() + 0.5)), int(np.floor(xs.mean() + 0.5)))
    # the bank crosses one, two, four and more than twelve 64-node blocks (the node counts the issue states)
    assert most > {(2, 64, 64): (100, 40), (2, 230, 97): (800, 200), (1, 129, 200): (900, 200)}[shape][L > 0], most


def test_the_banks_node_counts_cross_the_blocks():
    info = lambda *a: RU.bank_host(*a)[2][:, 0].tolist()      # noqa: E731
    assert info("smooth1.5~smooth3", (2, 230, 97), 0, 0) == [404, 395] and info("smooth1.5~smooth3", (2, 230, 97), 0, 1) == [139, 115]
    assert info("smooth1.5~smooth3", (2, 230, 97), 8, 0) == [196, 215] and info("smooth1.5~smooth3", (2, 230, 97), 8, 1) == [77, 79]
    assert info("rand0.45~rand0.55", (1, 129, 200), 0, 0) == [905] and info("rand0.45~rand0.55", (1, 129, 200), 0, 1) == [339]
    assert info("rand0.45~rand0.55", (2, 64, 64), 8, 0) == [46, 37] and info("rand0.45~rand0.55", (2, 64, 64), 8, 1) == [5, 13]


def _graph(pixels, rows, max_nodes=None, **kw):
    m, e, c = RU.direct(pixels, rows, **kw)
    return RU.host(m, e, c, 0, max_nodes or max(len(pixels), 1))


def test_hand_graphs():
    px = [40, 100, 333, 700, 1000]
    # a path 0 - 1 - 2 - 3: weights 70 * 3 + 99 * 2 = 408, 70, 99
    nodes, dist, info = _graph(px[:4], [(0, 1, 3, 2), (1, 2, 1, 0), (2, 3, 0, 1)])
    assert dist[0].tolist() == [[0, 408, 478, 577], [408, 0, 70, 169], [478, 70, 0, 99], [577, 169, 99, 0]] and info[0].tolist() == [4, 4, 3, 0]
    assert nodes[0].tolist() == [[-(q + 1), q // 32, q % 32, 1] for q in px[:4]]
    # a ring 0 - 1 - 2 - 3 - 4 - 0 of 10 orthogonal links each with a chord 1 - 3 of 5
    ring = [(i, (i + 1) % 5, 10, 0) for i in range(5)] + [(1, 3, 5, 0)]
    d = _graph(px, ring)[1][0] // 70
    assert d.tolist() == [[0, 10, 20, 15, 10], [10, 0, 10, 5, 15], [20, 10, 0, 10, 20], [15, 5, 10, 0, 10], [10, 15, 20, 10, 0]]
    # two parallel edges: the minimum wins, in either order of the rows; both are used
    for rows in ([(0, 1, 9, 0), (1, 0, 2, 1)], [(1, 0, 2, 1), (0, 1, 9, 0)]):
        nodes, dist, info = _graph(px[:2], rows)
        assert dist[0].tolist() == [[0, 239], [239, 0]] and info[0].tolist() == [2, 2, 2, 0]
    # a loop through one node is ignored and not counted; so is a ring (node_a == node_b == 0)
    m, e, c = (np.array(a) for a in RU.direct(px[:3], [(0, 1, 4, 0), (2, 2, 1, 0), (1, 1, 0, 0)]))
    e[0, 2, 4:6] = 0
    nodes, dist, info = RU.host(m, e, c, 0, 3)
    assert dist[0].tolist() == [[0, 280, INF], [280, 0, INF], [INF, INF, 0]] and info[0].tolist() == [3, 3, 1, 0]
    # a row of weight INF (and one far past it, formed in 64 bits) is no path; sums are cut at INF
    huge = (INF - 70 * 3) // 99 + 1
    assert 70 * 3 + 99 * (huge - 1) < INF <= 70 * 3 + 99 * huge
    nodes, dist, info = _graph(px[:4], [(0, 1, 3, huge), (1, 2, 0x7fffffff, 0x7fffffff), (2, 3, 3, huge - 1)])
    assert dist[0].tolist() == [[0, INF, INF, INF], [INF, 0, INF, INF], [INF, INF, 0, 210 + 99 * (huge - 1)], [INF, INF, 210 + 99 * (huge - 1), 0]]
    assert info[0].tolist() == [4, 4, 3, 0]
    # inconsistent rows are skipped and counted: a negative length, a node that the map does not hold
    m, e, c = (np.array(a) for a in RU.direct(px[:3], [(0, 1, -1, 0), (1, 2, 0, -5), (0, 2, 1, 1), (0, 1, 2, 2)]))
    e[0, 3, 5] = -5000
    nodes, dist, info = RU.host(m, e, c, 0, 3)
    assert info[0].tolist() == [3, 3, 1, 3] and dist[0].tolist() == [[0, INF, 169], [INF, 0, INF], [169, INF, 0]]
    # max_nodes below the nodes: the first rows stay, edges into dropped nodes are skipped; max_edges below the count: rows dropped
    nodes, dist, info = _graph(px, ring, max_nodes=3)
    assert info[0].tolist() == [5, 3, 2, 4] and (dist[0] // 70).tolist() == [[0, 10, 20], [10, 0, 10], [20, 10, 0]]
    nodes, dist, info = _graph(px, ring, cap=2, count=6)
    assert info[0].tolist() == [5, 5, 2, 0] and dist[0, 0, :].tolist() == [0, 700, 1400, INF, INF]
    # an empty image
    nodes, dist, info = RU.host(np.zeros((1, 3, 3), np.int32), np.zeros((1, 1, 8), np.int32), np.zeros((1, 4), np.int32), 1, 4)
    assert info.tolist() == [[0, 0, 0, 0]] and (nodes == RU.FILL).all() and (dist == RU.FILL).all()


@pytest.mark.parametrize("kind", sorted(RU.DIRECT_KINDS))
def test_direct_inputs_against_scipy(kind):
    for count in RU.DIRECT_COUNTS:
        m, e, c = RU.direct_case(kind, count)
        nodes, dist, info = RU.host(m, e, c, 0, 256)
        ref = RU.reference_distances(count, RU.DIRECT_KINDS[kind](count))
        assert np.array_equal(dist[0, :count, :count], ref) and info[0, :2].tolist() == [count, count], (kind, count)
        if kind == "split" and count > 1:
            assert (ref == INF).sum() == 2 * (count // 2) * (count - count // 2)
        if kind == "chain":
            assert (ref < INF).all()


def test_restatement_rejects_what_the_header_rejects():
    m, e, c = RU.direct([5, 9], [(0, 1, 1, 0)])
    hostio.graph_routes(m, e, c, 1, 1)
    hostio.graph_routes(m, e, c, 0, 1024)
    for kw in (dict(side=2), dict(side=-1), dict(side=True), dict(max_nodes=0), dict(max_nodes=1025), dict(max_nodes=2.0), dict(max_nodes=True),
               dict(node_map=m[0]), dict(node_map=m.astype(np.float32)), dict(edges=e[:, :, :7]), dict(edges=np.zeros((2, 1, 8), np.int32)),
               dict(counts=c[:, :3]), dict(node_map=np.zeros((1, 1025, 2), np.int32))):
        a = dict(node_map=m, edges=e, counts=c, side=0, max_nodes=4)
        a.update(kw)
        with pytest.raises(ValueError, match="graph_routes"):
            hostio.graph_routes(**a)
    g = hostio.graph_routes(m, e, c, 0, 4)
    hostio.route_score(*g, *g, 0)
    hostio.route_score(*g, *g, 1023)
    for bad in (-1, 1024, 1.0, True, None):
        with pytest.raises(ValueError, match="route_score"):
            hostio.route_score(*g, *g, bad)
    with pytest.raises(ValueError, match="route_score"):
        hostio.route_score(g[0], g[1], g[2], g[0][:, :3], g[1], g[2], 3)
    with pytest.raises(ValueError, match="route_score"):
        hostio.route_score(g[0], g[1].astype(np.float32), g[2], *g, 3)


# ------------------------------------------------------------------------------------------- the score
def test_a_graph_against_itself_scores_zero():
    """every node finds itself, unless another node of a smaller index holds the same position (a zone's rounded centroid on a line end of
    another road: the tie goes to the smaller index, by the header's rule); with the identity as match the sum of q is exactly 0"""
    pairs = 0
    for name in RU.BANK:
        for shape in RU.SHAPES:
            for L in SU.PRUNES:
                for side in (0, 1):
                    g = RU.bank_host(name, shape, L, side)
                    match, acc = RU.host_score(g, g)
                    distinct = True
                    for n in range(shape[0]):
                        k = int(g[2][n, 1])
                        pos = g[0][n, :k, 1:3]
                        first = np.array([int(np.nonzero((pos == q).all(axis=1))[0][0]) for q in pos], np.int64).reshape(-1)
                        assert match[n, :k].tolist() == first.tolist() and (match[n, k:] == RU.FILL).all(), (name, shape, L, side, n)
                        distinct &= first.tolist() == list(range(k))
                    pairs += int(acc[0])
                    if distinct:
                        assert acc[1:].tolist() == [0, 0, 0], (name, shape, L, side, acc)
                    assert acc[2] == 0 and acc[1] <= Q * acc[0]
    assert pairs > 100000


def test_scores_worked_out_by_hand():
    px = [40, 100, 333, 700]
    full = _graph(px, [(0, 1, 10, 0), (1, 2, 10, 0), (2, 3, 10, 0)])
    # an empty prediction: every pair of the truth is unmatched, the score of that direction is 0; the other direction has no pair
    none = RU.host(np.zeros((1, 32, 32), np.int32), np.zeros((1, 1, 8), np.int32), np.zeros((1, 4), np.int32), 0, 4)
    match, acc = RU.host_score(full, none)
    assert acc.tolist() == [6, 6 * Q, 6, 0] and match[0].tolist() == [-1] * 4
    match, acc = RU.host_score(none, full)
    assert acc.tolist() == [0, 0, 0, 0] and (match == RU.FILL).all()
    out = hostio.route_metrics(RU.host_score(full, none)[1], acc, np.array([0, 0, 0, 0, 4, 4, 3, 0]))
    assert (out["apls_true_to_pred"], out["apls_pred_to_true"], out["apls"]) == (0.0, 0.0, 0.0)
    # one edge replaced by a detour of twice its length: d = (10, 20, 30, 10, 20, 10) against e = (10, 30, 40, 20, 30, 10) in units of 70
    detour = _graph(px, [(0, 1, 10, 0), (1, 2, 20, 0), (2, 3, 10, 0)])
    q = [0, Q * 10 // 20, Q * 10 // 30, Q * 10 // 10, Q * 10 // 20, 0]
    assert q == [0, 32768, 21845, 65536, 32768, 0]
    match, acc = RU.host_score(full, detour)
    assert match[0].tolist() == [0, 1, 2, 3] and acc.tolist() == [6, sum(q), 0, 0]
    back = RU.host_score(detour, full)[1]
    assert back.tolist() == [6, 0 + Q * 10 // 30 + Q * 10 // 40 + Q * 10 // 20 + Q * 10 // 30 + 0, 0, 0]
    out = hostio.route_metrics(acc, back, np.array([4, 4, 3, 0, 4, 4, 3, 0]))
    t, b = 1.0 - sum(q) / (6.0 * Q), 1.0 - int(back[1]) / (6.0 * Q)
    assert out["apls_true_to_pred"] == t and out["apls_pred_to_true"] == b and out["apls"] == 2 * t * b / (t + b)
    # a broken counterpart: the prediction lacks the middle edge
    gap = _graph(px, [(0, 1, 10, 0), (2, 3, 10, 0)])
    assert RU.host_score(full, gap)[1].tolist() == [6, 4 * Q, 0, 4] and RU.host_score(gap, full)[1].tolist() == [2, 0, 0, 0]
    # a match tie goes to the smaller index: b's nodes at (1, 4) and (1, 8) are both 2 from a's node at (1, 6)
    a = _graph([32 + 6, 700], [(0, 1, 5, 0)], max_nodes=3)
    b = _graph([32 + 4, 32 + 8, 700], [(0, 2, 5, 0), (1, 2, 7, 0)], max_nodes=3)
    match, acc = RU.host_score(a, b, slack=2)
    assert match[0].tolist() == [0, 2, RU.FILL] and acc.tolist() == [1, 0, 0, 0]
    assert RU.host_score(a, b, slack=1)[0][0].tolist() == [-1, 2, RU.FILL]      # 2 > slack
    # slack = 0 matches equal positions only
    moved = _graph([41, 100, 333, 700], [(0, 1, 10, 0), (1, 2, 10, 0), (2, 3, 10, 0)])
    match, acc = RU.host_score(full, moved, slack=0)
    assert match[0].tolist() == [-1, 1, 2, 3] and acc.tolist() == [6, 3 * Q, 3, 0]
    assert RU.host_score(full, moved, slack=1)[1].tolist() == [6, 0, 0, 0]


def test_route_metrics_and_its_refusals():
    out = hostio.route_metrics(np.array([10, 5 * Q, 2, 1]), np.array([4, Q, 0, 0]), np.array([9, 7, 5, 1, 6, 6, 4, 0]))
    assert list(out) == ["apls_true_to_pred", "route_pairs_true_to_pred", "route_unmatched_true_to_pred", "route_broken_true_to_pred",
                         "apls_pred_to_true", "route_pairs_pred_to_true", "route_unmatched_pred_to_true", "route_broken_pred_to_true", "apls",
                         "graph_nodes_pred", "graph_nodes_dropped_pred", "graph_nodes_true", "graph_nodes_dropped_true"]
    assert out["apls_true_to_pred"] == 0.5 and out["apls_pred_to_true"] == 0.75 and out["apls"] == 2 * 0.5 * 0.75 / 1.25
    assert (out["route_pairs_true_to_pred"], out["route_unmatched_true_to_pred"], out["route_broken_true_to_pred"]) == (10, 2, 1)
    assert (out["graph_nodes_pred"], out["graph_nodes_dropped_pred"], out["graph_nodes_true"], out["graph_nodes_dropped_true"]) == (9, 2, 6, 0)
    zero = np.zeros(4, np.int64)
    assert hostio.route_metrics(zero, np.array([4, 0, 0, 0]), np.zeros(8, np.int64))["apls"] == 0.0      # a direction without a pair
    assert hostio.route_metrics(np.array([4, 0, 0, 0]), np.array([4, 0, 0, 0]), np.zeros(8, np.int64))["apls"] == 1.0
    for bad in (np.zeros(3, np.int64), np.zeros(4, np.float64), np.array([1, -1, 0, 0]), np.array([1, 2 * Q, 0, 0]), np.array([1, 0, 1, 1]), 5):
        with pytest.raises(ValueError, match="route_metrics"):
            hostio.route_metrics(bad, zero, np.zeros(8, np.int64))
        with pytest.raises(ValueError, match="route_metrics"):
            hostio.route_metrics(zero, bad, np.zeros(8, np.int64))
    for bad in (np.zeros(4, np.int64), np.zeros(8, np.float64), -np.ones(8, np.int64), np.array([1, 2, 0, 0, 0, 0, 0, 0])):
        with pytest.raises(ValueError, match="route_metrics"):
            hostio.route_metrics(zero, zero, bad)


# ------------------------------------------------------------------------------------------- the flags and the accumulator
def test_the_flags_and_their_refusals():
    defs = {d[0]: d for d in M.EXTRA_FLAG_DEFS}
    assert defs["validate_routes"][1:3] == (bool, False) and defs["max_graph_nodes"][1:3] == (int, 256) and defs["route_snap"][1:3] == (int, 8)
    assert defs["road_graph_distances"][1:3] == (bool, False) and "not a measurement" in defs["route_snap"][3]
    for o in (M.Options(), parse_options([])):
        assert (o.validate_routes, o.max_graph_nodes, o.route_snap, o.road_graph_distances) == (False, 256, 8, False)
    o = parse_options(["--validate_centerlines", "--validate_segments", "--validate_routes", "--max_graph_nodes=1024", "--route_snap=0",
                       "--save_best_metric=apls", "--save_road_graph", "--road_graph_distances"])
    assert (o.validate_routes, o.max_graph_nodes, o.route_snap, o.save_best_metric, o.road_graph_distances) == (True, 1024, 0, "apls", True)
    assert M.parse_save_best_metric("apls") == "apls" and M.parse_max_graph_nodes("7") == 7 and M.parse_route_snap(np.int64(1023)) == 1023
    with pytest.raises(ValueError, match="--validate_routes requires --validate_segments"):
        M.Options(validate_routes=True, validate_centerlines=True)
    with pytest.raises(ValueError, match="--validate_routes requires --validate_segments"):
        parse_options(["--validate_routes"])
    with pytest.raises(ValueError, match="--save_best_metric=apls requires --validate_routes"):
        M.Options(save_best_metric="apls", validate_centerlines=True, validate_segments=True)
    with pytest.raises(ValueError, match="--save_best_metric must be f1, relaxed_f1 or cl_quality"):      # the text still begins as it did
        M.parse_save_best_metric("dice")
    for bad in (0, -1, 1025, 2.5, True, None, "x"):
        with pytest.raises(ValueError, match="max_graph_nodes"):
            M.parse_max_graph_nodes(bad)
        with pytest.raises(ValueError, match="max_graph_nodes"):
            M.Options(max_graph_nodes=bad)
    for bad in (-1, 1024, 2.5, True, None, "x"):
        with pytest.raises(ValueError, match="route_snap"):
            M.parse_route_snap(bad)
        with pytest.raises(ValueError, match="route_snap"):
            M.Options(route_snap=bad)
    assert MM._WS["routes"][0] == "rsu_routes_ws_bytes"


def test_the_accumulators_new_stage():
    assert MM.Flags._fields[-1] == "routes" and len(MM.Flags._fields) == 7
    six = MM.Flags(True, True, True, 2, True, True)      # six arguments keep working: the stage is off
    assert not six.routes and "routes" not in MM.layout(six) and MM.total(six) == 4 + 128 + 133 + 140 + 20
    assert not MM.Flags(routes=True).routes and not MM.Flags(centerlines=True, routes=True).routes      # it counts only with segments
    on = MM.Flags(centerlines=True, segments=True, routes=True)
    lay = MM.layout(on)
    assert list(lay)[-3:] == ["routes", "routes.acc", "routes.info"] and lay["routes"] == slice(153, 169)
    assert lay["routes.acc"] == slice(153, 161) and lay["routes.info"] == slice(161, 169) and MM.total(on) == 169
    assert list(MM.STAGES)[-2:] == ["segments", "routes"] and MM.STAGES["routes"] == (("acc", 8), ("info", 8))

    class O:
        validate_centerlines, validate_segments, validate_routes = True, True, True
    assert MM.Flags.of(O()) == on
    c = np.zeros(169, np.float64)
    c[153:161] = [10, 5 * Q, 2, 1, 4, Q, 0, 0]
    c[161:169] = [9, 7, 5, 1, 6, 6, 4, 0]
    got = MM.decode(on, c, 3)
    want = hostio.route_metrics(np.array([10, 5 * Q, 2, 1]), np.array([4, Q, 0, 0]), np.array([9, 7, 5, 1, 6, 6, 4, 0]))
    assert list(got)[-len(want):] == list(want) and all(got[k] == v for k, v in want.items())
    off = MM.decode(MM.Flags(centerlines=True, segments=True), c[:153], 3)
    assert list(got)[:-len(want)] == list(off)      # with the flag off: the parent's keys and nothing else
