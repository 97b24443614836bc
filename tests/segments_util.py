"""What the road-segment tests share (tests/test_segments_host.py, test_gpu_segments.py, test_gpu_segments_fenced.py,
test_gpu_segments_large.py): the (prediction, truth) pairs of tests/graph_util.py, thinned and pruned at L in {0, 8} on the host, the host
references of hostio.line_segments computed once per case, hand-drawn masks, and the launch helper of include/rsu_segments.h. A plain module,
imported by name."""
import functools

import numpy as np

from tests import components_util as CU
from tests import graph_util as GU

THRESHOLD = GU.THRESHOLD
MAX_SIDE, MAX_EDGES = 1024, 65536   # rsu_segments.h RSU_SEGMENTS_MAX_SIDE, RSU_SEGMENTS_MAX_EDGES
BLOCK, TILE_W, TILE_H = 256, 64, 16  # csrc/segments.hip SG_BLOCK (the compaction's block), SG_TW x SG_TH (the classify tile)
CC_TILE = CU.TILE                   # the labelling's tile
FILL = -7                           # what the row tables hold before a launch: rows past min(count, max_edges) keep it
CAP = 2048                          # max_edges of the bank's cases: above every count of theirs
PRUNES = (0, 8)
# one pixel; less than a wave; one labelling tile; a pixel more / less on either axis; with the all-ignored image; five classify-tile
# columns by fifteen rows, all partial; the widest row and the tallest column (16 labelling tiles, four merge levels)
SHAPES = [(1, 1, 1), (1, 3, 5), (2, 64, 64), (1, 65, 63), (3, 63, 65), (2, 230, 97), (1, 129, 200), (1, 3, 1024), (1, 1024, 3)]
NAMES = ("edges_pred", "edges_true", "counts", "seg_pred", "seg_true", "node_pred", "node_true", "acc")


def shape_id(s):
    return CU.shape_id(s)


def launches(shape):
    """the launch count include/rsu_segments.h states: 8 + M"""
    t = max(-(-shape[1] // CC_TILE), -(-shape[2] // CC_TILE))
    return 8 + (t - 1).bit_length()


def ws_layout(N, H, W):
    """the layout of csrc/segments.hip: four float32 planes and three int32 arrays of [4 N][H][W], then [4 N][ceil(H W / BLOCK)] counts"""
    return -(-(4 * N * H * W * 16 + 4 * N * (-(-(H * W) // BLOCK)) * 4) // 8) * 8


@functools.lru_cache(maxsize=None)
def _pair_cached(name, shape, min_branch):
    from road_segmentation_unet_amd import hostio
    prob, labels = GU.pair(name, shape, True)
    if min_branch:
        prob, labels = hostio.skeleton_graph(prob, THRESHOLD, labels, min_branch)[:2]
    prob, labels = np.array(prob), np.array(labels)
    prob.setflags(write=False)
    labels.setflags(write=False)
    return prob, labels


def pair(name, shape, min_branch):
    """(prob float32, labels int64), [N, H, W] each, read-only and shared: the thinned pair of tests/graph_util.py pruned at min_branch"""
    return _pair_cached(name, tuple(shape), int(min_branch))


@functools.lru_cache(maxsize=None)
def host_pair(name, shape, min_branch, max_edges=CAP):
    """hostio.line_segments on pair(...): computed once, shared, read-only"""
    prob, labels = pair(name, shape, min_branch)
    return host(prob, labels, max_edges)


def host(prob, labels, max_edges=CAP, threshold=THRESHOLD):
    from road_segmentation_unet_amd import hostio
    out = hostio.line_segments(prob, threshold, labels, max_edges, fill=FILL)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


def of_masks(pred, true):
    """(prob, labels) of two bool [N, H, W]"""
    return CU.prob_of(pred), true.astype(np.int64)


# ------------------------------------------------------------------------------------------- hand-drawn masks
def plus(H, W, cy, cx, arm):
    m = np.zeros((H, W), bool)
    m[cy, cx - arm:cx + arm + 1] = m[cy - arm:cy + arm + 1, cx] = True
    return m


def diagonal(H, W):
    m = np.zeros((H, W), bool)
    n = min(H, W)
    m[np.arange(n), np.arange(n)] = True
    return m


def block_edge_lines(H=8, W=128):
    """two short lines whose roots (their first pixels in row-major order) are the last pixel of one compaction block and the first pixel of
    the next: indices BLOCK - 1 and BLOCK"""
    assert W < BLOCK and BLOCK % W == 0 and H * W > 2 * BLOCK
    m = np.zeros((H, W), bool)
    y0, x0 = divmod(BLOCK - 1, W)          # the last pixel of a row
    m[y0:y0 + 4, x0] = True                # downwards from it
    y1, x1 = divmod(BLOCK, W)              # the first pixel of the next row
    m[y1, x1:x1 + 5] = True
    return m


# ------------------------------------------------------------------------------------------- launches (GPU tests)
def ws_bytes(shape, max_edges=CAP):
    from road_segmentation_unet_amd._lib import lib
    return int(lib().rsu_segments_ws_bytes(shape[0], shape[1], shape[2], int(max_edges)))


def new_ws(shape, max_edges=CAP):
    """a workspace of the advertised size, filled with a pattern: the entry must not count on its contents"""
    import torch
    from tests import hiputil as hu
    need = ws_bytes(shape, max_edges)
    assert need > 0 and need % 8 == 0
    return torch.full((need // 8,), 0x7FA57FA57FA57FA5, dtype=torch.int64, device=hu.DEV)


def run_segments(prob_t, labels_t, shape, max_edges=CAP, want=(True, True, True, True), acc=None, want_acc=True, ws=None, threshold=THRESHOLD):
    """(edges_pred, edges_true, counts, seg_pred, seg_true, node_pred, node_true, acc), each a device tensor or None. want: which of
    seg_pred, seg_true, node_pred, node_true are asked for (labels_t None: no *_true output, edges_true included). The tables start as
    FILL, the maps and counts as a sentinel; acc: accumulated into when given, else a new zeroed one when want_acc."""
    import torch
    from road_segmentation_unet_amd._lib import call
    from tests import hiputil as hu
    ws = new_ws(shape, max_edges) if ws is None else ws
    N = shape[0]
    table = lambda: torch.full((N, max_edges, 8), FILL, dtype=torch.int32, device=hu.DEV)   # noqa: E731
    plane = lambda: torch.full(shape, -0x5A5A5A5A, dtype=torch.int32, device=hu.DEV)         # noqa: E731
    lab = labels_t is not None
    ep, et = table(), (table() if lab else None)
    counts = torch.full((N, 4), -0x5A5A5A5A, dtype=torch.int32, device=hu.DEV)
    sp = plane() if want[0] else None
    st = plane() if want[1] and lab else None
    np_ = plane() if want[2] else None
    nt = plane() if want[3] and lab else None
    if acc is None and want_acc:
        acc = torch.zeros((2, 8), dtype=torch.int64, device=hu.DEV)
    call("rsu_line_segments", hu.ptr(prob_t), float(threshold), hu.ptr(labels_t), int(max_edges), hu.ptr(ep), hu.ptr(et), hu.ptr(counts),
         hu.ptr(sp), hu.ptr(st), hu.ptr(np_), hu.ptr(nt), hu.ptr(acc), hu.ptr(ws), shape[0], shape[1], shape[2], hu.stream())
    return ep, et, counts, sp, st, np_, nt, acc


def same(got, want, what):
    """byte for byte; an output not asked for is None on the device side"""
    for name, g, w in zip(NAMES, got, want):
        if g is None:
            continue
        g = g.cpu().numpy()
        assert w is not None and g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g != w)
            raise AssertionError((what, name, len(bad), bad[:4].tolist(), g[tuple(bad[0])], w[tuple(bad[0])]))
