"""What the clDice tests share (tests/test_cldice_host.py, test_gpu_cldice.py, test_gpu_cldice_fenced.py): the torch restatement of the
published soft_skel / soft_cldice (max_pool2d plus autograd; float64 unless told otherwise), the three kinds of input -- tie-free, tied
and saturated -- and the launch helpers of the C entries of include/rsu_cldice.h. A plain module, imported by name."""
import numpy as np
import torch
import torch.nn.functional as Fn

from tests.head_util import _with_ignored

f32 = np.float32
SHAPES = [(3, 37, 41), (2, 70, 67), (1, 131, 130), (1, 5, 3), (1, 1, 1), (2, 1, 40), (2, 40, 1)]
CASES = [(s, k) for s in SHAPES for k in (3, 16)] + [((3, 37, 41), k) for k in (0, 1, 10)]
SCALE, SMOOTH = 0.7, 1.0


# ------------------------------------------------------------------------------------------- the torch restatement
def torch_erode(x):
    return torch.minimum(-Fn.max_pool2d(-x, (3, 1), 1, (1, 0)), -Fn.max_pool2d(-x, (1, 3), 1, (0, 1)))


def torch_dilate(x):
    return Fn.max_pool2d(x, 3, 1, 1)


def torch_skeleton(x, iters):
    """soft_skel of Shit et al. on [B, H, W] (each image its own channel-less plane: pooling never crosses an image)"""
    x = x[:, None]
    skel = torch.relu(x - torch_dilate(torch_erode(x)))
    for _ in range(iters):
        x = torch_erode(x)
        d = torch.relu(x - torch_dilate(torch_erode(x)))
        skel = skel + torch.relu(d - skel * d)
    return skel[:, 0]


def torch_cldice(prob, labels, iters, scale, smooth, dtype=torch.float64):
    """(skel_p, skel_y, sums, gprob, term) by autograd; gprob is 0 at ignored pixels, whose p is a constant"""
    p0 = torch.tensor(np.asarray(prob), dtype=dtype)
    lab = torch.from_numpy(np.asarray(labels))
    m = ((lab == 0) | (lab == 1))
    leaf = p0.clone().requires_grad_(True)
    p = torch.where(m, leaf, p0)
    y = (lab == 1).to(dtype)
    mf = m.to(dtype)
    sp, sy = torch_skeleton(p, iters), torch_skeleton(y, iters)
    A, Bp, Cc, Dy = (mf * sp * y).sum(), (mf * sp).sum(), (mf * sy * p).sum(), (mf * sy).sum()
    Tp, Ts = (A + smooth) / (Bp + smooth), (Cc + smooth) / (Dy + smooth)
    term = scale * (1.0 - 2.0 * Tp * Ts / (Tp + Ts))
    term.backward()
    return (sp.detach().numpy(), sy.detach().numpy(), np.array([float(v.detach()) for v in (A, Bp, Cc, Dy)]), leaf.grad.numpy(),
            float(term.detach()))


# ------------------------------------------------------------------------------------------- inputs
def _base(B, H, W):
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    return np.stack([np.exp(-(y - 0.7 * x - 3 * b) ** 2 / 18) + np.exp(-(x - 0.6 * W) ** 2 / 8) + 0 * y for b in range(B)])


def _labels(rng, base, ignored):
    labels = (base > 0.5).astype(np.int64)
    if ignored and labels.size >= 200:   # (_with_ignored wants room for its six special labels)
        labels = _with_ignored(rng, labels.reshape(-1))[0].reshape(labels.shape)
    elif ignored:
        labels.reshape(-1)[::3] = -1
    return labels


def tie_free(shape, seed=0, ignored=True):
    """(p float32, labels int64): ranks keep every value of p distinct in float32"""
    B, H, W = shape
    n = B * H * W
    rng = np.random.RandomState(seed)
    base = _base(B, H, W)
    f = 0.85 * np.clip(base, 0, 1) + 0.1 * (rng.permutation(n).reshape(shape) + 0.5) / n
    rank = np.argsort(np.argsort(f.reshape(-1), kind="stable"), kind="stable").reshape(shape)
    p = (0.02 + 0.96 * (rank + 0.5) / n).astype(f32)
    assert np.unique(p).size == n
    return p, _labels(rng, base, ignored)


def tied(shape, lev, seed=0, ignored=True):
    """maps quantised to lev + 1 levels, every value doubled along a row: ties in every window"""
    rng = np.random.RandomState(seed + lev)
    p = (rng.randint(0, lev + 1, size=shape) / lev).astype(f32)
    p = np.maximum(p, np.roll(p, 1, axis=2))
    return p, _labels(rng, _base(*shape), ignored)


def saturated(shape, seed=0, ignored=True):
    """exactly 1.0 over the road interiors, exactly 0.0 far from them, the tie-free values between"""
    p, labels = tie_free(shape, seed, ignored)
    base = _base(*shape)
    p = np.where(base > 0.5, f32(1), np.where(base < 0.1, f32(0), p)).astype(f32)
    return p, labels


INPUTS = {"tie_free": tie_free, "tied4": lambda s: tied(s, 4), "tied16": lambda s: tied(s, 16), "saturated": saturated}


# ------------------------------------------------------------------------------------------- the aux head's reference
class AuxRef:
    """tests/focal_util.Ref (gamma = 0: the weighted cross-entropy of tests/head_util.Ref) with the linear term sum gprob_i p_i over the
    counted pixels added to the objective, gprob given: float64 torch autograd on the CPU"""

    def __init__(self, act, w, b, labels, class_w, pixel_w, inv, gamma, gprob, lam=0.0, smooth=1.0):
        from oracle import unet_oracle as U
        t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=True)  # noqa: E731
        A, W, Bv = t(act), t(w), t(b)
        valid = (labels == 0) | (labels == 1)
        y = torch.from_numpy((labels == 1).astype(np.float64))
        pw = np.ones(labels.size, np.float64) if pixel_w is None else np.asarray(pixel_w, np.float64)
        mass = torch.from_numpy(np.where(valid, pw, 0.0))
        cw = np.ones(2) if class_w is None else np.asarray(class_w, np.float64)
        omega = torch.from_numpy(np.where(valid, cw[np.where(valid, labels, 0)] * pw, 0.0))
        gp = torch.from_numpy(np.where(valid, np.asarray(gprob, np.float64), 0.0))   # (by selection: an ignored pixel's gprob may be inf or nan)
        z = A @ W + Bv
        logp = torch.log_softmax(z, dim=1)
        p = torch.exp(logp[:, 1])
        ce = -torch.where(y > 0, logp[:, 1], logp[:, 0])
        focal = torch.exp(float(gamma) * torch.where(y > 0, logp[:, 0], logp[:, 1]))
        loss = torch.sum(torch.where(omega != 0, omega * focal * ce, torch.zeros_like(ce)))
        I, P, Y = torch.sum(mass * p * y), torch.sum(mass * p), torch.sum(mass * y)
        dice_term = lam * (1.0 - (2.0 * I + smooth) / (P + Y + smooth)) if lam else 0.0
        (loss * inv + dice_term + torch.sum(gp * p)).backward()
        self.prob = p.detach().numpy()
        self.loss_sum, self.wsum = float(loss.detach()), float(omega.sum())
        self.sums = np.array([float(I.detach()), float(P.detach()), float(Y.detach())])
        self.dact = U.relu_bwd(act, A.grad.numpy().astype(np.float32))
        self.dw, self.db = W.grad.numpy(), Bv.grad.numpy()


# ------------------------------------------------------------------------------------------- launches (GPU tests)
def ws_floats(shape, iters):
    from road_segmentation_unet_amd._lib import lib
    return int(lib().rsu_cldice_ws_floats(shape[0], shape[1], shape[2], iters))


def run_fwd(bufs, iters, shape, st):
    from road_segmentation_unet_amd._lib import call
    from tests import hiputil as hu
    call("rsu_cldice_fwd", hu.ptr(bufs["prob"]), hu.ptr(bufs["labels"]), iters, hu.ptr(bufs["skel_p"]), hu.ptr(bufs["skel_y"]),
         hu.ptr(bufs["sums"]), hu.ptr(bufs["ws"]), shape[0], shape[1], shape[2], st)


def run_bwd(bufs, iters, scale, smooth, shape, st, sums="sums"):
    from road_segmentation_unet_amd._lib import call
    from tests import hiputil as hu
    call("rsu_cldice_bwd", hu.ptr(bufs["prob"]), hu.ptr(bufs["labels"]), hu.ptr(bufs["skel_p"]), hu.ptr(bufs["skel_y"]), hu.ptr(bufs[sums]),
         iters, scale, smooth, hu.ptr(bufs["gprob"]), hu.ptr(bufs["ws"]), shape[0], shape[1], shape[2], st)
