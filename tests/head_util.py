"""What the -m gpu tests of the head family share (tests/test_gpu_weighted_loss.py, test_gpu_dice_loss.py, test_gpu_validation.py): test_head's
inputs, weight maps and ignored labels, the float64 torch reference of the weighted cross-entropy + soft-Dice head, and the small
networks / models above it. A plain module, imported by name."""
import numpy as np
import torch

from oracle import unet_oracle as U
from tests import hiputil as hu

RSU_EINVAL = -22   # include/rsu.h
NPIX = 3 * 37 * 41
LAM, SMOOTH = 0.7, 1.0
NETS = [(3, 16, True, 20), (2, 16, False, 20)]


def _rand(rng, *shape, scale=1.0):
    return (rng.standard_normal(shape) * scale).astype(np.float32)


def _inputs(C):
    """test_head's inputs"""
    rng = np.random.RandomState(C)
    act = hu.q(np.maximum(_rand(rng, NPIX, C), 0))
    w = _rand(rng, C, 2, scale=0.3)
    b = _rand(rng, 2, scale=0.1)
    labels = (rng.rand(NPIX) < 0.2).astype(np.int64)
    return rng, act, w, b, labels


def _weight_map(rng, n=NPIX):
    pw = (0.25 + rng.rand(n)).astype(np.float32)
    pw[rng.rand(n) < 0.05] = 0.0
    return pw


def _with_ignored(rng, labels):
    """~10 % ignored labels: -1, a few 255, and one 2**32 + 1 (its low 32 bits are a valid label)"""
    labels = labels.copy()
    ign = rng.rand(labels.size) < 0.10
    labels[ign] = -1
    few = rng.choice(np.nonzero(~ign)[0], 6, replace=False)
    labels[few[:5]] = 255
    labels[few[5]] = 2 ** 32 + 1
    ign = (labels != 0) & (labels != 1)
    assert ign.sum() > labels.size // 20
    return labels, ign


def _bits(t):
    """the tensor's bits as integers (bit-for-bit comparisons: -0 != +0, NaNs compare by payload)"""
    return t.contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else torch.int32)


def _dev_labels(labels):
    return torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int64)).to(hu.DEV)


class Ref:
    """float64 torch on the CPU: z = act w + b, p = softmax(z)[1], CE, the Dice sums, and autograd of
    sum omega CE inv + lam (1 - D). With `sums` given, D and U are those constants and the Dice term is its linearisation
    lam sum m (D - 2 y) / U p -- whose gradient is the formula of rsu.h evaluated with those sums."""

    def __init__(self, act, w, b, labels, class_w, pixel_w, inv, lam=LAM, smooth=SMOOTH, sums=None):
        t = lambda a: torch.tensor(np.asarray(a, np.float64), dtype=torch.float64, requires_grad=True)  # noqa: E731
        A, W, Bv = t(act), t(w), t(b)
        valid = (labels == 0) | (labels == 1)
        y = torch.from_numpy((labels == 1).astype(np.float64))
        pw = np.ones(labels.size, np.float64) if pixel_w is None else np.asarray(pixel_w, np.float64)
        mass = torch.from_numpy(np.where(valid, pw, 0.0))             # (by selection: an ignored pixel's pixel_w may be inf or nan)
        cw = np.ones(2) if class_w is None else np.asarray(class_w, np.float64)
        omega = torch.from_numpy(np.where(valid, cw[np.where(valid, labels, 0)] * pw, 0.0))
        z = A @ W + Bv
        logp = torch.log_softmax(z, dim=1)
        p = torch.exp(logp[:, 1])
        ce = -torch.where(y > 0, logp[:, 1], logp[:, 0])
        ce_sum = torch.sum(torch.where(omega != 0, omega * ce, torch.zeros_like(ce)))
        I, P, Y = torch.sum(mass * p * y), torch.sum(mass * p), torch.sum(mass * y)
        self.sums = np.array([float(I.detach()), float(P.detach()), float(Y.detach())])
        if sums is None:
            D = (2.0 * I + smooth) / (P + Y + smooth)
            dice_term = lam * (1.0 - D)
        else:
            Ug = sums[1] + sums[2] + smooth
            Dg = (2.0 * sums[0] + smooth) / Ug
            dice_term = lam * torch.sum(mass * (Dg - 2.0 * y) / Ug * p)
        (ce_sum * inv + dice_term).backward()
        self.prob = p.detach().numpy()
        self.ce_sum, self.wsum = float(ce_sum.detach()), float(omega.sum())
        self.dact = U.relu_bwd(act, A.grad.numpy().astype(np.float32))
        self.dw, self.db = W.grad.numpy(), Bv.grad.numpy()
        self.valid = valid


def _net(L, root, dilated, P, class_weights=None, B=2, **kw):
    from road_segmentation_unet_amd.unet import UNet
    return UNet(L, root, dilated, B, P, seed=17, training=True, class_weights=class_weights, **kw)


def _batch(m, seed=6):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    m.x.copy_(torch.rand((m.B, m.S, m.S, 3), generator=gen))
    m.labels.copy_((torch.rand((m.B, m.P, m.P), generator=gen) < 0.3).to(torch.int64))


def _step(m, **kw):
    m.forward_device()
    m.backward_device(1.0 / (m.B * m.P * m.P), **kw)
    torch.cuda.synchronize()
    return m.flat_g.clone(), m.prob.clone(), m.loss_sum.clone(), m.weight_sum.clone(), m.dice_sums.clone()


def _model(**kw):
    from road_segmentation_unet_amd.model import ConvolutionalModel, Options
    o = dict(num_layers=3, root_size=16, patch_size=20, batch_size=2, dilated_layers=True, dropout=1.0, lr=0.01, seed=5, logdir=None)
    o.update(kw)
    return ConvolutionalModel(Options(**o), device="cuda:0", params=U.init_params(3, 16, True, seed=13, bias_scale=0.05))
