"""What the network-distance tests share (tests/test_routes_host.py, test_gpu_routes.py, test_gpu_routes_fenced.py,
test_gpu_routes_large.py): the inputs of include/rsu_routes.h taken from hostio.line_segments on the thinned pairs of
tests/segments_util.py, direct inputs (line ends only and hand-written edge rows, so that the distance kernels are tested apart from the
image chain), the host references of hostio.graph_routes and hostio.route_score computed once per case, the stated workspace layout and
launch count, and the launch helpers of the two entries. A plain module, imported by name."""
import functools

import numpy as np

from tests import segments_util as SU

MAX_SIDE, MAX_NODES, MAX_EDGES = 1024, 1024, 65536   # rsu_routes.h RSU_ROUTES_MAX_SIDE, RSU_ROUTES_MAX_NODES; the largest max_edges
INF, Q = 0x3fffffff, 65536                           # rsu_routes.h RSU_ROUTES_INF, RSU_ROUTES_Q
BLOCK, TILE = 256, 64                                # csrc/routes.hip RT_BLOCK, RT_TILE
FILL = -11           # what nodes, dist and match hold before a launch: elements the entries do not touch keep it
SENTINEL = -0x5A5A5A5A   # what info holds before a launch: it is written whole
SLACK = 8
NAMES = ("nodes", "dist", "info")
BANK = ("smooth1.5~smooth3", "smooth3~smooth6", "rand0.45~rand0.55", "holed~lone2x2")
SHAPES = [(2, 64, 64), (2, 230, 97), (1, 129, 200)]
DIRECT_SIDE = 32     # the direct inputs' image: DIRECT_SIDE x DIRECT_SIDE, a line end at chosen pixels


def rounds(max_nodes):
    """T = ceil(max_nodes / 64), the rounds of the blocked Floyd-Warshall"""
    return -(-max_nodes // TILE)


def launches(max_nodes):
    """the launch count include/rsu_routes.h states for rsu_graph_routes: 8 + 2 T"""
    return 8 + 2 * rounds(max_nodes)


def ws_layout(N, H, W, max_nodes):
    """the layout include/rsu_routes.h states: int32 [N][ceil(H W / 256)], then int32 [N][max_nodes][3]"""
    return 4 * (N * (-(-(H * W) // BLOCK)) + N * max_nodes * 3)


def _frozen(arrays):
    for a in arrays:
        a.setflags(write=False)
    return tuple(arrays)


@functools.lru_cache(maxsize=None)
def bank_inputs(name, shape, min_branch, side):
    """(node_map, edges, counts) of one side of hostio.line_segments on the thinned pair `name` pruned at min_branch: shared, read-only"""
    out = SU.host_pair(name, tuple(shape), min_branch)
    return out[5 + side], out[side], out[2]


def host(node_map, edges, counts, side, max_nodes):
    from road_segmentation_unet_amd import hostio
    return _frozen(hostio.graph_routes(node_map, edges, counts, side, max_nodes, fill=FILL))


@functools.lru_cache(maxsize=None)
def bank_host(name, shape, min_branch, side, max_nodes=MAX_NODES):
    return host(*bank_inputs(name, shape, min_branch, side), side, max_nodes)


def host_score(a, b, slack=SLACK):
    from road_segmentation_unet_amd import hostio
    return _frozen(hostio.route_score(*a, *b, slack, fill=FILL))


@functools.lru_cache(maxsize=None)
def bank_score(name, shape, min_branch, a_side, max_nodes=MAX_NODES, slack=SLACK):
    """(match, acc) from side a_side to the other side of the pair"""
    return host_score(bank_host(name, shape, min_branch, a_side, max_nodes), bank_host(name, shape, min_branch, 1 - a_side, max_nodes), slack)


# ------------------------------------------------------------------------------------------- direct inputs
def direct(pixels, rows, cap=None, count=None):
    """(node_map int32 [1, 32, 32], edges int32 [1, cap, 8], counts int32 [1, 4]) of line ends at the row-major indices `pixels` (node k of
    the table is the k-th smallest) and the rows (a, b, ortho, diag) between nodes a and b of that numbering; counts of both sides say
    `count` (default: the rows)"""
    pixels = sorted(int(p) for p in pixels)
    assert len(set(pixels)) == len(pixels) and 0 <= pixels[0] and pixels[-1] < DIRECT_SIDE * DIRECT_SIDE
    m = np.zeros(DIRECT_SIDE * DIRECT_SIDE, np.int32)
    m[pixels] = -(np.asarray(pixels, np.int32) + 1)
    cap = max(len(rows), 1) if cap is None else cap
    e = np.full((1, cap, 8), SU.FILL, np.int32)
    for r, (a, b, ortho, diag) in enumerate(rows[:cap]):
        ia, ib = -(pixels[a] + 1), -(pixels[b] + 1)
        e[0, r] = (r + 1, min(max(ortho + diag + 1, 1), 1 << 20), ortho, diag, min(ia, ib), max(ia, ib), 0, 2)
    n = len(rows) if count is None else count
    return _frozen((m.reshape(1, DIRECT_SIDE, DIRECT_SIDE), e, np.array([[n, 0, n, 0]], np.int32)))


def spread(count, seed=0):
    """`count` distinct pixels of the direct image, ascending"""
    rng = np.random.RandomState(1000 + 7 * count + seed)
    return np.sort(rng.choice(DIRECT_SIDE * DIRECT_SIDE, count, replace=False)).tolist()


def chain_rows(count, seed=0):
    """a chain through all `count` nodes in a shuffled order: its shortest paths cross every block of the table"""
    order = np.random.RandomState(50 + count + seed).permutation(count)
    return [(int(a), int(b), 1 + (i * 7) % 13, (i * 5) % 11) for i, (a, b) in enumerate(zip(order[:-1], order[1:]))]


def sparse_rows(count, seed=0):
    """about 2 count random rows over `count` nodes: parallel rows, loops through one node and zero weights among them"""
    rng = np.random.RandomState(90 + count + seed)
    return [(int(rng.randint(count)), int(rng.randint(count)), int(rng.randint(0, 40)), int(rng.randint(0, 40))) for _ in range(2 * count)]


def split_rows(count, seed=0):
    """two chains over the two halves of the table (interleaved): no path between them"""
    even, odd = list(range(0, count, 2)), list(range(1, count, 2))
    return [(a, b, 3, 2) for part in (even, odd) for a, b in zip(part[:-1], part[1:])]


DIRECT_KINDS = {"chain": chain_rows, "sparse": sparse_rows, "split": split_rows}
DIRECT_COUNTS = (1, 2, 63, 64, 65, 128, 129, 200)


@functools.lru_cache(maxsize=None)
def direct_case(kind, count):
    return direct(spread(count), DIRECT_KINDS[kind](count))


def reference_distances(count, rows):
    """all-pairs path lengths over `count` nodes and rows (a, b, ortho, diag) by scipy's Dijkstra, written apart from hostio's: int64
    [count, count], INF where there is no path"""
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import shortest_path
    best = {}
    for a, b, ortho, diag in rows:
        if a != b:
            w = min(70 * ortho + 99 * diag, INF)
            best[(a, b)] = best[(b, a)] = min(w, best.get((a, b), INF))
    out = np.full((count, count), INF, np.int64)
    if best:      # a zero weight is an edge, which a sparse matrix cannot hold: every weight + 1 / (2 count), exact in float64 below 2^53
        keys = list(best)
        eps = 1.0 / (2 * count)
        g = csr_matrix(([best[k] + eps for k in keys], ([k[0] for k in keys], [k[1] for k in keys])), shape=(count, count))
        d = shortest_path(g, method="D", directed=True)
        finite = np.isfinite(d)
        out[finite] = np.floor(d[finite]).astype(np.int64)
    out[np.arange(count), np.arange(count)] = 0
    return np.minimum(out, INF)


# ------------------------------------------------------------------------------------------- launches (GPU tests)
def ws_bytes(shape, max_nodes):
    from road_segmentation_unet_amd._lib import lib
    return int(lib().rsu_routes_ws_bytes(shape[0], shape[1], shape[2], int(max_nodes)))


def new_ws(shape, max_nodes):
    """a workspace of the advertised size, filled with a pattern: the entry must not count on its contents"""
    import torch
    from tests import hiputil as hu
    need = ws_bytes(shape, max_nodes)
    assert need > 0 and need % 4 == 0
    return torch.full((need // 4,), 0x7FA57FA5, dtype=torch.int32, device=hu.DEV)


def dev(a):
    import torch
    from tests import hiputil as hu
    return torch.from_numpy(np.array(a)).to(hu.DEV)   # (a copy: the shared arrays are read-only)


def run_routes(map_t, edges_t, counts_t, side, max_nodes, ws=None):
    """(nodes, dist, info) as device tensors. nodes and dist start as FILL, info as a sentinel"""
    import torch
    from road_segmentation_unet_amd._lib import call
    from tests import hiputil as hu
    shape, cap = tuple(map_t.shape), int(edges_t.shape[1])
    ws = new_ws(shape, max_nodes) if ws is None else ws
    N = shape[0]
    full = lambda s, v: torch.full(s, v, dtype=torch.int32, device=hu.DEV)   # noqa: E731
    nodes, dist, info = full((N, max_nodes, 4), FILL), full((N, max_nodes, max_nodes), FILL), full((N, 4), SENTINEL)
    call("rsu_graph_routes", hu.ptr(map_t), hu.ptr(edges_t), hu.ptr(counts_t), int(side), cap, int(max_nodes), hu.ptr(nodes), hu.ptr(dist),
         hu.ptr(info), hu.ptr(ws), shape[0], shape[1], shape[2], hu.stream())
    return nodes, dist, info


def run_score(a, b, slack=SLACK, acc=None):
    """(match, acc) as device tensors from two graphs (nodes, dist, info) of device tensors; match starts as FILL; acc: accumulated into
    when given, else a new zeroed one"""
    import torch
    from road_segmentation_unet_amd._lib import call
    from tests import hiputil as hu
    N, max_nodes = int(a[0].shape[0]), int(a[0].shape[1])
    match = torch.full((N, max_nodes), FILL, dtype=torch.int32, device=hu.DEV)
    acc = torch.zeros(4, dtype=torch.int64, device=hu.DEV) if acc is None else acc
    call("rsu_route_score", hu.ptr(a[0]), hu.ptr(a[1]), hu.ptr(a[2]), hu.ptr(b[0]), hu.ptr(b[1]), hu.ptr(b[2]), max_nodes, int(slack),
         hu.ptr(match), hu.ptr(acc), N, hu.stream())
    return match, acc


def same(got, want, what, names=NAMES):
    """byte for byte"""
    for name, g, w in zip(names, got, want):
        g = g.cpu().numpy()
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g != w)
            raise AssertionError((what, name, len(bad), bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))


def check(node_map, edges, counts, side, max_nodes, what, want=None):
    """rsu_graph_routes on the device against hostio.graph_routes; returns (got, want)"""
    want = host(node_map, edges, counts, side, max_nodes) if want is None else want
    got = run_routes(dev(node_map), dev(edges), dev(counts), side, max_nodes)
    same(got, want, what)
    return got, want


def check_score(got_a, got_b, want, what, slack=SLACK):
    """rsu_route_score on two device graphs against (match, acc) of hostio.route_score"""
    same(run_score(got_a, got_b, slack), want, what, ("match", "acc"))
