"""What the focal-loss tests share (tests/test_focal_host.py, test_gpu_focal.py, test_gpu_loss_fenced.py): the float64 torch-autograd
reference of the focal heads of include/rsu_loss.h -- tests/head_util.Ref with omega * exp(gamma * logp_o) * CE in place of omega * CE,
the same Dice handling and the same relu_bwd on dact -- and a numpy float32 restatement of the header's rule, operation by operation, for
the host tests. A plain module, imported by name."""
import numpy as np
import torch

from oracle import unet_oracle as U
from tests.head_util import LAM, SMOOTH

f32 = np.float32
GAMMAS = (0.5, 2.0, 5.0)
CLASS_W = (0.6, 2.5)
SATURATE = 60.0     # _inputs(C)'s w times this: p_o and p_t underflow to exactly 0 in float32 at hundreds of pixels


class Ref:
    """float64 torch on the CPU: z = act w + b, logp = log_softmax(z), CE = -logp_t, F = exp(gamma logp_o), and autograd of
    sum omega F CE inv + lam (1 - D); `sums` as in head_util.Ref. Labels other than 0 / 1 ignore their pixel by selection."""

    def __init__(self, act, w, b, labels, class_w, pixel_w, inv, gamma, lam=0.0, smooth=SMOOTH, sums=None):
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
        focal = torch.exp(float(gamma) * torch.where(y > 0, logp[:, 0], logp[:, 1]))
        loss = torch.sum(torch.where(omega != 0, omega * focal * ce, torch.zeros_like(ce)))
        I, P, Y = torch.sum(mass * p * y), torch.sum(mass * p), torch.sum(mass * y)
        self.sums = np.array([float(I.detach()), float(P.detach()), float(Y.detach())])
        if lam == 0.0:
            dice_term = 0.0
        elif sums is None:
            dice_term = lam * (1.0 - (2.0 * I + smooth) / (P + Y + smooth))
        else:
            Ug = sums[1] + sums[2] + smooth
            Dg = (2.0 * sums[0] + smooth) / Ug
            dice_term = lam * torch.sum(mass * (Dg - 2.0 * y) / Ug * p)
        (loss * inv + dice_term).backward()
        self.prob = p.detach().numpy()
        self.logits = z.detach().numpy()
        self.loss_sum, self.wsum = float(loss.detach()), float(omega.sum())
        self.ce_sum = self.loss_sum       # (the name head_util.Ref's users read)
        self.dact = U.relu_bwd(act, A.grad.numpy().astype(np.float32))
        self.dw, self.db = W.grad.numpy(), Bv.grad.numpy()
        self.valid = valid


def _fma(a, b, c):
    """one rounding (the float64 product of two float32 is exact; the sum's double rounding is rarer than 1e-8)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)


def rule_f32(logits, labels, gamma, omega, inv):
    """include/rsu_loss.h's rule restated in numpy float32, every operation one rounding, from float32 logits [n, 2]: the softmax of the
    heads (m, e, s, p = e / s), CE = -(l_t - m - log s), F = exp2(gamma * log2(p_o)), the pixel's loss omega * (F * CE) and
    g = (omega * inv) * (F * fma(gamma * p_t, CE, p_o)). Returns (p1, loss terms, dlogits [n, 2]); 0 by selection where the label is
    neither 0 nor 1."""
    l = np.asarray(logits, f32)
    labels = np.asarray(labels)
    valid = (labels == 0) | (labels == 1)
    lab = np.where(valid, labels, 0).astype(np.int64)
    gamma, inv = f32(gamma), f32(inv)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        m = np.maximum(l[:, 0], l[:, 1])
        e0, e1 = np.exp(l[:, 0] - m), np.exp(l[:, 1] - m)
        s = e0 + e1
        p0, p1 = e0 / s, e1 / s
        pt, po = np.where(lab == 1, p1, p0), np.where(lab == 1, p0, p1)
        ce = -((np.where(lab == 1, l[:, 1], l[:, 0]) - m) - np.log(s))
        F = np.exp2(gamma * np.log2(po))
        fce = F * ce
        fg = F * _fma(gamma * pt, ce, po)
        om = np.where(valid, np.asarray(omega, f32), f32(0))
        g = (om * inv) * fg
        terms = np.where(valid, om * fce, f32(0)).astype(f32)
    g = np.where(valid, g, f32(0)).astype(f32)
    d = np.zeros_like(l)
    d[:, 0] = np.where(lab == 1, g, -g)
    d[:, 1] = np.where(lab == 1, -g, g)
    d[~valid] = 0
    return p1, terms, d


def omega_of(labels, class_w, pixel_w):
    """class_w[label] * pixel_w as float32, 0 at ignored labels"""
    valid = (labels == 0) | (labels == 1)
    om = np.ones(labels.size, f32)
    if class_w is not None:
        om = om * np.asarray(class_w, f32)[np.where(valid, labels, 0)]
    if pixel_w is not None:
        om = om * np.where(valid, np.asarray(pixel_w, f32), f32(1))
    return np.where(valid, om, f32(0)).astype(f32)


__all__ = ["Ref", "rule_f32", "omega_of", "GAMMAS", "CLASS_W", "SATURATE", "LAM", "SMOOTH"]
