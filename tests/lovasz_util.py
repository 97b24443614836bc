"""What the Lovasz tests share (tests/test_lovasz_host.py, test_gpu_lovasz.py, test_gpu_lovasz_fenced.py): an independent float64 torch
statement of the loss (Berman's lovasz_grad on |y - p|, torch.sort, per image, autograd), the bounds of a float32 sum in the mirror's and
in the kernels' order, the bank of inputs and the launch helpers of include/rsu_lovasz.h. A plain module, imported by name."""
import math

import numpy as np
import torch

f32 = np.float32
U32 = 2.0 ** -24          # the unit roundoff of float32
TILE = 4096               # lovasz.h LV_TILE
SCALE = 0.7


# ------------------------------------------------------------------------------------------- the torch statement
def lovasz_grad(gt_sorted):
    """Berman, Triki and Blaschko: the gradient of the Lovasz extension of the Jaccard loss w.r.t. sorted errors"""
    p = len(gt_sorted)
    gts = gt_sorted.sum()
    intersection = gts - gt_sorted.cumsum(0)
    union = gts + (1 - gt_sorted).cumsum(0)
    jaccard = 1.0 - intersection / union
    if p > 1:
        jaccard[1:p] = jaccard[1:p] - jaccard[0:-1]
    return jaccard


def torch_lovasz(prob, labels, scale, dtype=torch.float64):
    """(per-image losses [B], d (scale / B sum_b L_b) / d prob, g_k of every counted pixel at its place) by autograd; pixels whose
    label is neither 0 nor 1 take no part"""
    p = torch.tensor(np.asarray(prob), dtype=dtype, requires_grad=True)
    lab = torch.from_numpy(np.asarray(labels))
    B = p.shape[0]
    losses = []
    for b in range(B):
        pb, lb = p[b].reshape(-1), lab[b].reshape(-1)
        m = (lb == 0) | (lb == 1)
        if not bool(m.any()):
            losses.append(pb.sum() * 0.0)
            continue
        y = lb[m].to(dtype)
        e = (y - pb[m]).abs()
        es, perm = torch.sort(e, dim=0, descending=True)
        losses.append(torch.dot(es, lovasz_grad(y[perm])))
    total = torch.stack(losses).sum() * (float(scale) / B)
    total.backward()
    return np.array([float(v.detach()) for v in losses]), p.grad.numpy()


# ------------------------------------------------------------------------------------------- bounds of the float32 sums
def _gamma(d):
    return d * U32 / (1.0 - d * U32)


def host_depth(n):
    """additions on the longest path of numpy's pairwise float32 sum of n terms: blocks of at most 128 terms in 8 strided accumulators
    (16 additions), 3 to combine them, one per halving above a block"""
    return 19 + max(0, int(math.ceil(math.log2(max(n, 1) / 128.0)))) + 1


def gpu_depth(shape):
    """rsu_lovasz.h: a thread's 8 ranks in order (8 additions, the first onto 0), a tree over 512 threads (9), of an image's tiles thread
    i of 256 adds every 256th in order and a tree adds the threads (8), the images in order (B)"""
    B, H, W = shape
    pn = TILE
    while pn < H * W:
        pn *= 2
    return 8 + 9 + int(math.ceil(pn / TILE / 256.0)) + 8 + B


def sum_bound(depth, total):
    """|float32 sum - exact sum| of non-negative terms whose exact sum is `total`, `depth` additions on the longest path"""
    return 1.001 * _gamma(depth) * abs(total)


# ------------------------------------------------------------------------------------------- inputs
def _labels(rng, shape, road=0.2):
    return (rng.rand(*shape) < road).astype(np.int64)


def random_case(shape, seed=0):
    """p uniform in (0, 1), independent of the labels; about 20 % road"""
    rng = np.random.RandomState(seed)
    return rng.rand(*shape).astype(f32), _labels(rng, shape)


def quant4(shape, seed=1):
    """p quantised to four values: massive ties between pixels of different labels"""
    rng = np.random.RandomState(seed)
    return (rng.randint(0, 4, size=shape) / 4.0 + 0.125).astype(f32), _labels(rng, shape, 0.4)


def all_equal(shape, seed=2):
    rng = np.random.RandomState(seed)
    return np.full(shape, 0.37, f32), _labels(rng, shape, 0.3)


def no_road(shape, seed=3):
    p, _ = random_case(shape, seed)
    return p, np.zeros(shape, np.int64)


def all_road(shape, seed=4):
    p, _ = random_case(shape, seed)
    return p, np.ones(shape, np.int64)


def image_ignored(shape, seed=5):
    """every label of image 0 ignored, beside normal images (B = 1: nothing is counted at all)"""
    p, labels = random_case(shape, seed)
    labels[0] = -1
    return p, labels


def scattered_ignored(shape, seed=6):
    """about 10 % of the labels ignored: 2, -1 and 1 << 32 (its low 32 bits are a valid label)"""
    p, labels = random_case(shape, seed)
    rng = np.random.RandomState(seed + 100)
    r = rng.rand(*shape)
    labels[r < 0.10] = -1
    labels[r < 0.06] = 2
    labels[r < 0.03] = 1 << 32
    return p, labels


def special(shape, seed=7):
    """p holding 0, 1, values outside [0, 1], infinities and one NaN: the order is defined on bit patterns"""
    p, labels = random_case(shape, seed)
    flat = p.reshape(-1)
    vals = [0.0, 1.0, -0.25, 1.5, np.inf, -np.inf, 0.0, 1.0, -0.0, 3.0]
    rng = np.random.RandomState(seed + 100)
    pos = rng.permutation(flat.size)
    for j, v in enumerate(vals[:max(0, flat.size - 1)]):
        flat[pos[j]] = v
    if flat.size > len(vals):
        flat[pos[len(vals)]] = np.nan
    return p, labels


INPUTS = {"random": random_case, "quant4": quant4, "all_equal": all_equal, "no_road": no_road, "all_road": all_road,
          "image_ignored": image_ignored, "scattered_ignored": scattered_ignored, "special": special}


def tie_free(shape, seed=0):
    """(p, labels) whose errors |y - p| are pairwise distinct in float32: e = m / 2^20 with distinct integers m, p = e or 1 - e (exact)"""
    rng = np.random.RandomState(seed)
    n = int(np.prod(shape))
    m = rng.permutation((1 << 20) - 1)[:n] + 1
    e = (m / float(1 << 20)).astype(f32).reshape(shape)
    labels = _labels(rng, shape, 0.3)
    p = np.where(labels == 1, f32(1) - e, e).astype(f32)
    return p, labels


# ------------------------------------------------------------------------------------------- launches (GPU tests)
def ws_bytes(shape):
    from road_segmentation_unet_amd._lib import lib
    return int(lib().rsu_lovasz_ws_bytes(*shape))


def run_fwd_bwd(bufs, scale, accumulate, shape, st):
    from road_segmentation_unet_amd._lib import call
    from tests import hiputil as hu
    call("rsu_lovasz_fwd_bwd", hu.ptr(bufs["prob"]), hu.ptr(bufs["labels"]), scale, accumulate, hu.ptr(bufs["gprob"]), hu.ptr(bufs["loss"]),
         hu.ptr(bufs["ws"]), shape[0], shape[1], shape[2], st)


def run_fwd(bufs, shape, st, loss="loss"):
    from road_segmentation_unet_amd._lib import call
    from tests import hiputil as hu
    call("rsu_lovasz_fwd", hu.ptr(bufs["prob"]), hu.ptr(bufs["labels"]), hu.ptr(bufs[loss]), hu.ptr(bufs["ws"]), shape[0], shape[1], shape[2], st)
