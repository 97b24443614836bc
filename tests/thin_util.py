"""What the thinning tests share (tests/test_thin_host.py, test_gpu_thin.py, test_gpu_thin_fenced.py, test_gpu_thin_large.py): the bank of
masks, the (prediction, truth) pairs built from it, the host references of hostio computed once per case, topology counts by scipy and the
launch helper of include/rsu_thin.h. A plain module, imported by name."""
import functools

import numpy as np

from tests import components_util as CU

f32 = np.float32
THRESHOLD = CU.THRESHOLD
MAX_SIDE, MAX_ITERS = 1024, 512     # rsu_thin.h RSU_THIN_MAX_SIDE, RSU_THIN_MAX_ITERS
K, CORE, CROWS = 8, 32, 96          # csrc/thin.h TH_K; the tile of a step launch: 64 - 4 K pixels wide, TH_ROWS - 4 K = 128 - 32 rows high
ITERS = (1, K - 1, K, K + 1, 64)    # truncated in the first launch, at its end, one past it; the default
# (N, H, W): one pixel; less than a ballot word; one ballot word, one less / more; exactly one tile, a pixel less / more on either axis;
# three row tiles by four word columns, all partial; two by seven; the widest row (32 words) and the tallest column (11 row tiles)
SHAPES = [(1, 1, 1), (1, 3, 5), (2, 64, 64), (1, 65, 63), (3, 63, 65), (2, CROWS, CORE), (1, CROWS + 1, CORE - 1), (3, CROWS - 1, CORE + 1),
          (2, 230, 97), (1, 129, 200), (1, 3, 1024), (1, 1024, 3)]
# one solid 100 x 100 block laid across the corners of tiles (row 96, columns 32, 64 and 96): about 56 iterations to its fixed point
BLOCK_SHAPE = (1, 170, 110)


def shape_id(s):
    return CU.shape_id(s)


def _rand(d):
    return lambda H, W, rng: rng.random_sample((H, W)) < d


def _smooth(sigma):
    def make(H, W, rng):
        from scipy import ndimage
        return ndimage.gaussian_filter(rng.standard_normal((H, W)), sigma) > 0.0
    return make


def _holed(H, W, rng):
    """a solid block a pixel inside the image with a rectangular hole in it"""
    m = np.zeros((H, W), bool)
    m[1:H - 1, 1:W - 1] = True
    m[H // 3:H // 3 + max(H // 4, 1), W // 4:W // 4 + max(W // 3, 1)] = False
    return m


def _lone(H, W, rng):
    m = np.zeros((H, W), bool)
    m[H // 2:H // 2 + 2, W // 2:W // 2 + 2] = True
    return m


MASKS = {"rand0.3": _rand(0.3), "rand0.45": _rand(0.45), "rand0.55": _rand(0.55), "rand0.7": _rand(0.7), "rand0.9": _rand(0.9),
         "smooth1.5": _smooth(1.5), "smooth3": _smooth(3.0), "smooth6": _smooth(6.0), "ones": lambda H, W, rng: np.ones((H, W), bool),
         "zeros": lambda H, W, rng: np.zeros((H, W), bool), "holed": _holed, "lone2x2": _lone}
KINDS = sorted(MASKS)


@functools.lru_cache(maxsize=None)
def _masks_cached(kind, shape):
    N, H, W = shape
    out = np.stack([MASKS[kind](H, W, np.random.RandomState(1000 * KINDS.index(kind) + n)) for n in range(N)])
    out.setflags(write=False)
    return out


def masks(kind, shape):
    """bool [N, H, W] (read-only, shared between the tests); the images of a stack differ where the kind is random"""
    return _masks_cached(kind, tuple(shape))


def block_mask():
    m = np.zeros(BLOCK_SHAPE, bool)
    m[0, 62:162, 2:102] = True
    return m


def pair_names():
    """every kind as the prediction against the next kind as the truth: each kind is thinned on both sides"""
    return ["%s~%s" % (k, KINDS[(i + 1) % len(KINDS)]) for i, k in enumerate(KINDS)]


@functools.lru_cache(maxsize=None)
def _pair_cached(name, shape):
    a, b = name.split("~")
    prob, labels = CU.prob_of(masks(a, shape)), masks(b, shape).astype(np.int64)
    prob.setflags(write=False)
    labels.setflags(write=False)
    return prob, labels


def pair(name, shape):
    """(prob float32, labels int64), [N, H, W] each, read-only and shared: prob's mask at THRESHOLD is the first kind, labels the second"""
    return _pair_cached(name, tuple(shape))


@functools.lru_cache(maxsize=None)
def host_pair(name, shape, max_iters):
    """(skel_pred, skel_true, counts, info) of hostio.mask_thin on pair(name, shape): computed once, shared, read-only"""
    from road_segmentation_unet_amd import hostio
    prob, labels = pair(name, shape)
    out = hostio.mask_thin(prob, THRESHOLD, labels, max_iters)
    for a in out:
        a.setflags(write=False)
    return out


def mixed_labels(shape, seed=23):
    """int64 labels [N, H, W]: smooth road blobs, about 9 % ignored (-1, 2 and (1 << 32) | 1, whose low 32 bits are a valid road label) and,
    with more than one image, the last image ignored altogether (the padding of an evaluation chunk)"""
    rng = np.random.RandomState(seed)
    lab = masks("smooth3", shape).astype(np.int64)
    r = rng.random_sample(shape)
    lab[r < 0.09] = -1
    lab[r < 0.06] = 2
    lab[r < 0.03] = (1 << 32) | 1
    if shape[0] > 1:
        lab[-1] = -1
    return lab


# ------------------------------------------------------------------------------------------- topology, by scipy
def topology(mask2d):
    """(8-connected foreground components, 4-connected background components of the mask padded by one background pixel)"""
    from scipy import ndimage
    fg = ndimage.label(mask2d, structure=np.ones((3, 3), int))[1]
    bg = ndimage.label(~np.pad(mask2d, 1))[1]
    return int(fg), int(bg)


# ------------------------------------------------------------------------------------------- launches (GPU tests)
def ws_bytes(shape, max_iters):
    from road_segmentation_unet_amd._lib import lib
    return int(lib().rsu_thin_ws_bytes(shape[0], shape[1], shape[2], int(max_iters)))


def new_ws(shape, max_iters):
    """a workspace of the advertised size, filled with a pattern: the entry must not count on its contents"""
    import torch
    from tests import hiputil as hu
    need = ws_bytes(shape, max_iters)
    assert need > 0 and need % 8 == 0
    return torch.full((need // 8,), 0x7FA57FA57FA57FA5, dtype=torch.int64, device=hu.DEV)


def run_thin(prob_t, labels_t, shape, max_iters, want_pred=True, want_true=True, acc=None, want_acc=True, want_info=True, ws=None,
             threshold=THRESHOLD):
    """(skel_pred or None, skel_true or None, acc or None, info or None) as device tensors; labels_t may be None (then want_true must be
    False). acc: accumulated into when given, else a new zeroed one when want_acc and both outputs are asked for"""
    import torch
    from road_segmentation_unet_amd._lib import call
    from tests import hiputil as hu
    ws = new_ws(shape, max_iters) if ws is None else ws
    sp = torch.full(shape, float("nan"), dtype=torch.float32, device=hu.DEV) if want_pred else None
    st = torch.full(shape, -7, dtype=torch.int64, device=hu.DEV) if want_true else None
    if acc is None and want_acc and want_pred and want_true:
        acc = torch.zeros(4, dtype=torch.int64, device=hu.DEV)
    info = torch.full((shape[0], 2), -7, dtype=torch.int32, device=hu.DEV) if want_info else None
    call("rsu_mask_thin", hu.ptr(prob_t), float(threshold), hu.ptr(labels_t), int(max_iters), hu.ptr(sp), hu.ptr(st), hu.ptr(acc), hu.ptr(info),
         hu.ptr(ws), shape[0], shape[1], shape[2], hu.stream())
    return sp, st, acc, info
