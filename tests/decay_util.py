"""The decaying update pass of include/rsu_optim.h restated in numpy float32 -- every operation one IEEE rounding, in the header's order
-- for both rules (Momentum, Adam) and both modes (l2, decoupled), and the same steps as float64 formulas for the host tests to hold the
restatement against. `decays` False is the plain rule: what the pass does to a plain range (biases, colour adjust, the 1x1 head)."""
import numpy as np

F = np.float32
L2, DECOUPLED = 0, 1   # rsu_optim.h RSU_DECAY_L2, RSU_DECAY_DECOUPLED


def momentum(w, a, g, lr, mu, gs):
    """rsu.h rsu_update_table_run on one variable: (w, acc) after the step; gs = gscale (times the clipping factor)"""
    a1 = F(mu) * a + F(gs) * g
    return w - F(lr) * a1, a1


def adam(w, m, v, g, alpha, beta1, beta2, epsilon, gs):
    """rsu.h rsu_update_table_run_adam on one variable: (w, m, v) after the step"""
    g1 = F(gs) * g
    m1 = m + (g1 - m) * (F(1) - F(beta1))
    v1 = v + (g1 * g1 - v) * (F(1) - F(beta2))
    return w - (m1 * F(alpha)) / (np.sqrt(v1) + F(epsilon)), m1, v1


def decayed_weights(w, decay):
    """the decoupled step: w - (f32(decay) * w), two float32 roundings"""
    return w - F(decay) * w


def l2_gradient(w, g, gs, decay, decays=True):
    """the gradient the l2 mode hands to its rule (with 1 for gscale): (gs * g) + (decay * w); a plain range: gs * g"""
    g1 = F(gs) * g
    return g1 + F(decay) * w if decays else g1


def momentum_decay(w, a, g, lr, mu, gs, decay, mode, decays=True):
    if not decays:
        return momentum(w, a, g, lr, mu, gs)
    if mode == DECOUPLED:
        return momentum(decayed_weights(w, decay), a, g, lr, mu, gs)
    return momentum(w, a, l2_gradient(w, g, gs, decay), lr, mu, 1.0)


def adam_decay(w, m, v, g, alpha, beta1, beta2, epsilon, gs, decay, mode, decays=True):
    if not decays:
        return adam(w, m, v, g, alpha, beta1, beta2, epsilon, gs)
    if mode == DECOUPLED:
        return adam(decayed_weights(w, decay), m, v, g, alpha, beta1, beta2, epsilon, gs)
    return adam(w, m, v, l2_gradient(w, g, gs, decay), alpha, beta1, beta2, epsilon, 1.0)


# ---- the same in float64, as formulas (the scalars are the float32 values the kernel receives)
def momentum_decay_f64(w, a, g, lr, mu, gs, decay, mode):
    w, a, g = (np.asarray(t, np.float64) for t in (w, a, g))
    lr, mu, gs, decay = (float(F(s)) for s in (lr, mu, gs, decay))
    if mode == DECOUPLED:
        a1 = mu * a + gs * g
        return (1.0 - decay) * w - lr * a1, a1
    a1 = mu * a + gs * g + decay * w
    return w - lr * a1, a1


def adam_decay_f64(w, m, v, g, alpha, beta1, beta2, epsilon, gs, decay, mode):
    w, m, v, g = (np.asarray(t, np.float64) for t in (w, m, v, g))
    alpha, beta1, beta2, epsilon, gs, decay = (float(F(s)) for s in (alpha, beta1, beta2, epsilon, gs, decay))
    g1 = gs * g + (decay * w if mode == L2 else 0.0)
    m1 = beta1 * m + (1.0 - beta1) * g1
    v1 = beta2 * v + (1.0 - beta2) * g1 * g1
    w0 = (1.0 - decay) * w if mode == DECOUPLED else w
    return w0 - alpha * m1 / (np.sqrt(v1) + epsilon), m1, v1
