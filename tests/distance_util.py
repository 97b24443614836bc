"""What the mask-distance tests share (tests/test_distance_host.py, test_gpu_distance.py, test_gpu_distance_fenced.py,
test_gpu_distance_large.py): the bank of (prediction, truth) pairs built from the masks of tests/components_util.py, the host references
of hostio computed once per case, and the launch helpers of include/rsu_distance.h. A plain module, imported by name."""
import functools

import numpy as np

from tests import components_util as CU

f32 = np.float32
THRESHOLD = CU.THRESHOLD
BINS, NONE, MAX_SIDE = 64, 0x7fffffff, 1024     # rsu_distance.h RSU_DIST_BINS, RSU_DIST_NONE, RSU_DIST_MAX_SIDE
# the shapes of tests/components_util.py (one pixel; one row and one column of two 64-pixel chunks; a chunk less / more than a pixel; three
# chunks by two strips, both partial; 150 x 150) and the staging limits: the widest row, the tallest column (16 chunks)
SHAPES = CU.SHAPES + [(1, 3, 1024), (1, 1024, 3)]
ALL_BINS_SHAPE = (2, 130, 150)   # an all-ones prediction against one true pixel at the corner: every bin of acc[0], the last one included
SHIFT = (3, -2)


def shape_id(s):
    return CU.shape_id(s)


def shifted(mask, dy, dx):
    """mask [N, H, W] moved by (dy, dx) inside every image, False moving in"""
    N, H, W = mask.shape
    out = np.zeros_like(mask)
    ys, yd = (slice(0, max(H - dy, 0)), slice(dy, H)) if dy >= 0 else (slice(-dy, H), slice(0, max(H + dy, 0)))
    xs, xd = (slice(0, max(W - dx, 0)), slice(dx, W)) if dx >= 0 else (slice(-dx, W), slice(0, max(W + dx, 0)))
    out[:, yd, xd] = mask[:, ys, xs]
    return out


def _single(shape, image, first):
    m = np.zeros(shape, bool)
    m[image, 0 if first else -1, 0 if first else -1] = True
    return m


def pair_names(shape):
    """the names of the (prediction, truth) pairs of one shape"""
    names = ["%s~shift" % k for k in CU.KINDS] + ["spiral~rings", "rand0.41~empty", "empty~rand0.41"]
    if shape[0] > 1:
        names.append("neighbours")
    if tuple(shape) == ALL_BINS_SHAPE:
        names.append("full~corner")
    return names


@functools.lru_cache(maxsize=None)
def _pair_cached(name, shape):
    a, b = name.split("~") if "~" in name else (name, None)
    if name == "neighbours":   # image 0: one predicted pixel at its last pixel; image 1: one true pixel at its first. Neighbours in memory only
        pred, true = _single(shape, 0, False), _single(shape, 1, True)
    elif name == "full~corner":
        pred, true = np.ones(shape, bool), np.zeros(shape, bool)
        true[:, 0, 0] = True
    elif b == "shift":
        true = CU.masks(a, shape)
        pred = shifted(true, *SHIFT)
    else:
        pred, true = CU.masks(a, shape), CU.masks(b, shape)
    prob, labels = CU.prob_of(pred), true.astype(np.int64)
    prob.setflags(write=False)
    labels.setflags(write=False)
    return prob, labels


def pair(name, shape):
    """(prob float32, labels int64), [N, H, W] each, read-only and shared: prob's mask at THRESHOLD is the prediction, labels are 0 / 1"""
    return _pair_cached(name, tuple(shape))


def mixed_labels(shape, seed=19):
    """int64 labels [N, H, W]: about half road, about 9 % ignored (-1, 2 and (1 << 32) | 1, whose low 32 bits are a valid road label) and,
    with more than one image, the last image ignored altogether (the padding of an evaluation chunk)"""
    rng = np.random.RandomState(seed)
    lab = (rng.random_sample(shape) < 0.5).astype(np.int64)
    r = rng.random_sample(shape)
    lab[r < 0.09] = -1
    lab[r < 0.06] = 2
    lab[r < 0.03] = (1 << 32) | 1
    if shape[0] > 1:
        lab[-1] = -1
    return lab


# ------------------------------------------------------------------------------------------- references
def scipy_d2(mask):
    """int64 [H, W]: scipy's Euclidean distance transform to `mask`, squared and rounded (exact on these sizes: checked against the
    brute-force minimum in tests/test_distance_host.py); NONE for an empty mask"""
    from scipy import ndimage
    if not mask.any():
        return np.full(mask.shape, NONE, np.int64)
    return np.rint(ndimage.distance_transform_edt(~mask) ** 2).astype(np.int64)


def brute_d2(mask):
    """int64 [H, W]: min over the mask's pixels of dy^2 + dx^2, by trying them all"""
    H, W = mask.shape
    ys, xs = np.nonzero(mask)
    if ys.size == 0:
        return np.full(mask.shape, NONE, np.int64)
    qy, qx = np.mgrid[0:H, 0:W]
    out = np.full((H, W), NONE, np.int64)
    for s in range(0, ys.size, 256):
        d = (qy[..., None] - ys[s:s + 256]) ** 2 + (qx[..., None] - xs[s:s + 256]) ** 2
        np.minimum(out, d.min(axis=-1), out=out)
    return out


def masks_of(prob, labels, threshold=THRESHOLD):
    """(P, T) by the header's definitions, written out once more for the tests"""
    with np.errstate(invalid="ignore"):
        above = np.asarray(prob, f32) >= f32(threshold)
    if labels is None:
        return above, np.zeros(above.shape, bool)
    labels = np.asarray(labels)
    return above & ((labels == 0) | (labels == 1)), labels == 1


@functools.lru_cache(maxsize=None)
def host_pair(name, shape):
    """(d2_pred, d2_true, hist) of hostio on pair(name, shape): computed once, shared, read-only"""
    from road_segmentation_unet_amd import hostio
    prob, labels = pair(name, shape)
    out = hostio.mask_distance(prob, THRESHOLD, labels) + (hostio.distance_hist(prob, THRESHOLD, labels),)
    for a in out:
        a.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------- launches (GPU tests)
def ws_bytes(shape):
    from road_segmentation_unet_amd._lib import lib
    return int(lib().rsu_distance_ws_bytes(*shape))


def new_ws(shape):
    """a workspace of the advertised size, filled with a pattern: the entries must not count on its contents"""
    import torch
    from tests import hiputil as hu
    return torch.full((ws_bytes(shape) // 4,), 0x7FA57FA5, dtype=torch.int32, device=hu.DEV)


def run_mask_distance(prob_t, labels_t, shape, want_pred=True, want_true=True, ws=None, threshold=THRESHOLD):
    """(d2_pred or None, d2_true or None) as device tensors; labels_t may be None (then want_true must be False)"""
    import torch
    from road_segmentation_unet_amd._lib import call
    from tests import hiputil as hu
    ws = new_ws(shape) if ws is None else ws
    d2p = torch.full(shape, -7, dtype=torch.int32, device=hu.DEV) if want_pred else None
    d2t = torch.full(shape, -7, dtype=torch.int32, device=hu.DEV) if want_true else None
    call("rsu_mask_distance", hu.ptr(prob_t), float(threshold), hu.ptr(labels_t), hu.ptr(d2p), hu.ptr(d2t), hu.ptr(ws), shape[0], shape[1],
         shape[2], hu.stream())
    return d2p, d2t


def run_hist(prob_t, labels_t, shape, acc=None, ws=None, threshold=THRESHOLD):
    """acc (int64 [2, 64] on the device; a new zeroed one when not given) after one more rsu_distance_hist"""
    import torch
    from road_segmentation_unet_amd._lib import call
    from tests import hiputil as hu
    ws = new_ws(shape) if ws is None else ws
    acc = torch.zeros((2, BINS), dtype=torch.int64, device=hu.DEV) if acc is None else acc
    call("rsu_distance_hist", hu.ptr(prob_t), float(threshold), hu.ptr(labels_t), hu.ptr(acc), hu.ptr(ws), shape[0], shape[1], shape[2],
         hu.stream())
    return acc
