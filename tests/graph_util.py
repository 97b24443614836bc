"""What the centre-line graph tests share (tests/test_graph_host.py, test_gpu_graph.py, test_gpu_graph_fenced.py, test_gpu_graph_large.py):
the (prediction, truth) pairs of tests/thin_util.py's bank, raw and pre-thinned, the host references of hostio.skeleton_graph computed once
per case, hand-drawn lines with spurs and rings, and the launch helper of include/rsu_graph.h. A plain module, imported by name."""
import functools

import numpy as np

from tests import components_util as CU
from tests import thin_util as TU

f32 = np.float32
THRESHOLD = TU.THRESHOLD
MAX_SIDE, MAX_BRANCH = 1024, 64     # rsu_graph.h RSU_GRAPH_MAX_SIDE, RSU_GRAPH_MAX_BRANCH
R, CORE, CROWS = 16, 32, 96         # csrc/graph.h GR_R; the tile of a step launch: 64 - 2 R pixels wide, GR_ROWS - 2 R = 128 - 32 rows high
# no prune step; one round; truncated in the first delete launch, at its end (the first regrow launch then carries R - 1 of R rounds),
# one past it; three delete launches; the limit
BRANCHES = (0, 1, R - 1, R, R + 1, 2 * R + 1, MAX_BRANCH)
# (N, H, W): one pixel; less than a ballot word; one ballot word; exactly one tile, a pixel less / more on either axis; three row tiles by
# four word columns, all partial; two by seven; the widest row (32 words) and the tallest column (11 row tiles)
SHAPES = [(1, 1, 1), (1, 3, 5), (2, 64, 64), (1, 65, 63), (3, 63, 65), (2, CROWS, CORE), (1, CROWS + 1, CORE - 1), (3, CROWS - 1, CORE + 1),
          (2, 230, 97), (1, 129, 200), (1, 3, 1024), (1, 1024, 3)]
CORNER_SHAPE = (1, 2 * CROWS - 20, 4 * CORE - 10)   # the corner of four tiles at row CROWS, column CORE, and three more down the row


def shape_id(s):
    return CU.shape_id(s)


def launches(min_branch):
    """the launch count include/rsu_graph.h states"""
    L = int(min_branch)
    return 2 if L == 0 else 2 + -(-L // R) + -(-(L + 1) // R)


@functools.lru_cache(maxsize=None)
def thinned(kind, shape):
    """the bank's masks thinned to their fixed point on the host: bool [N, H, W], read-only and shared"""
    from road_segmentation_unet_amd import hostio
    out = hostio.thin_mask(TU.masks(kind, shape), TU.MAX_ITERS)[0]
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _pair_cached(name, shape, pre_thinned):
    a, b = name.split("~")
    get = thinned if pre_thinned else TU.masks
    prob, labels = CU.prob_of(get(a, shape)), get(b, shape).astype(np.int64)
    prob.setflags(write=False)
    labels.setflags(write=False)
    return prob, labels


def pair(name, shape, pre_thinned):
    """(prob float32, labels int64), [N, H, W] each, read-only and shared: prob's mask at THRESHOLD is the first kind, labels the second"""
    return _pair_cached(name, tuple(shape), bool(pre_thinned))


@functools.lru_cache(maxsize=None)
def host_pair(name, shape, pre_thinned, min_branch):
    """(out_pred, out_true, junc_pred, junc_true, counts) of hostio.skeleton_graph on pair(...): computed once, shared, read-only"""
    from road_segmentation_unet_amd import hostio
    prob, labels = pair(name, shape, pre_thinned)
    out = hostio.skeleton_graph(prob, THRESHOLD, labels, min_branch)
    for a in out:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------- hand-drawn masks [H, W]
def line_with_spurs(H, W, y, x0, x1, spurs, step=8, first=None):
    """a horizontal line on row y from column x0 to x1 (inclusive) with vertical spurs of the given lengths, alternately above and below
    the line, `step` columns apart from column `first` (x0 + step by default) on"""
    m = np.zeros((H, W), bool)
    m[y, x0:x1 + 1] = True
    x = x0 + step if first is None else first
    for k, n in enumerate(spurs):
        if k % 2 == 0:
            m[y - n:y, x] = True
        else:
            m[y + 1:y + 1 + n, x] = True
        x += step
    assert x - step <= x1 and m.sum() == x1 + 1 - x0 + sum(spurs)
    return m


def ring(H, W, y0, x0, y1, x1):
    """a one-pixel rectangular ring with corners (y0, x0) and (y1, x1)"""
    m = np.zeros((H, W), bool)
    m[y0, x0:x1 + 1] = m[y1, x0:x1 + 1] = True
    m[y0:y1 + 1, x0] = m[y0:y1 + 1, x1] = True
    return m


def corner_line():
    """spurs of 1 .. 2 R + 2 pixels, three columns apart, on a line along the last core row above the corner of four tiles: the line and
    its spurs cross the tile borders at row CROWS and at columns CORE, 2 CORE and 3 CORE. The line runs from edge to edge: its own ends
    are 2 R + 3 and more pixels away from every spur but the first few"""
    N, H, W = CORNER_SHAPE
    spurs = list(range(1, 2 * R + 3))
    m = line_with_spurs(H, W, CROWS - 1, 0, W - 1, spurs, step=3, first=8)
    return m[None]


def corner_ring():
    N, H, W = CORNER_SHAPE
    return ring(H, W, CROWS - 30, CORE - 20, CROWS + 25, 3 * CORE + 7)[None]


# ------------------------------------------------------------------------------------------- launches (GPU tests)
def ws_bytes(shape, min_branch):
    from road_segmentation_unet_amd._lib import lib
    return int(lib().rsu_graph_ws_bytes(shape[0], shape[1], shape[2], int(min_branch)))


def new_ws(shape, min_branch):
    """a workspace of the advertised size, filled with a pattern: the entry must not count on its contents"""
    import torch
    from tests import hiputil as hu
    need = ws_bytes(shape, min_branch)
    assert need > 0 and need % 8 == 0
    return torch.full((need // 8,), 0x7FA57FA57FA57FA5, dtype=torch.int64, device=hu.DEV)


def run_graph(prob_t, labels_t, shape, min_branch, want=(True, True, True, True), acc=None, want_acc=True, ws=None, threshold=THRESHOLD,
              in_place=False):
    """(out_pred, out_true, junc_pred, junc_true, acc), each a device tensor or None; want: which of the four outputs are asked for
    (labels_t None: no *_true output). acc: accumulated into when given, else a new zeroed one when want_acc. in_place: out_pred is
    prob_t and out_true is labels_t themselves"""
    import torch
    from road_segmentation_unet_amd._lib import call
    from tests import hiputil as hu
    ws = new_ws(shape, min_branch) if ws is None else ws
    new_f = lambda: torch.full(shape, float("nan"), dtype=torch.float32, device=hu.DEV)   # noqa: E731
    new_i = lambda: torch.full(shape, -7, dtype=torch.int64, device=hu.DEV)               # noqa: E731
    op = (prob_t if in_place else new_f()) if want[0] else None
    ot = (labels_t if in_place else new_i()) if want[1] else None
    jp = new_f() if want[2] else None
    jt = new_i() if want[3] else None
    if acc is None and want_acc:
        acc = torch.zeros(8, dtype=torch.int64, device=hu.DEV)
    call("rsu_skeleton_graph", hu.ptr(prob_t), float(threshold), hu.ptr(labels_t), int(min_branch), hu.ptr(op), hu.ptr(ot), hu.ptr(jp),
         hu.ptr(jt), hu.ptr(acc), hu.ptr(ws), shape[0], shape[1], shape[2], hu.stream())
    return op, ot, jp, jt, acc
