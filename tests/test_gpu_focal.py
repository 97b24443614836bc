"""-m gpu: the focal cross-entropy heads (rsu_loss.h rsu_head_fwd_bwd_focal, rsu_head_eval_focal) through the C ABI against float64 torch
autograd (tests/focal_util.Ref) on test_head's inputs, on saturated logits, their bit relations with the other heads of the family
(gamma = 0, prob, weight_sum, training against evaluation, ignored pixels, determinism), the argument errors, the rounding of dact, and
the network / model level above them. Tolerances are tests/test_gpu_ops.py::test_head's as tests/test_gpu_weighted_loss.py and
tests/test_gpu_dice_loss.py use them; 2e-5 relative for scalar sums."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import focal_util as FU  # noqa: E402
from tests import hiputil as hu  # noqa: E402
from tests.head_util import (LAM, NETS, NPIX, RSU_EINVAL, SMOOTH, _batch, _bits, _dev_labels, _inputs, _model, _net, _step,  # noqa: E402
                             _weight_map, _with_ignored)
from road_segmentation_unet_amd._lib import RsuError, call, lib  # noqa: E402
from road_segmentation_unet_amd.model import focal_loss_terms  # noqa: E402

CW = FU.CLASS_W
INV = 1.0 / (2 * NPIX)
MODES = ["plain", "class", "map", "both", "ignored"]


class Out:
    """every output of the two entries (and of the Dice sums pass in front of the training entry)"""

    def __init__(self, C, fill=0.0, acc=0.0):
        z = lambda *s, dtype=torch.float32, v=fill: torch.full(s, v, dtype=dtype, device=hu.DEV)  # noqa: E731
        self.prob_a, self.sums = z(NPIX), z(3)
        self.prob, self.dact = z(NPIX), z(NPIX, C, dtype=torch.bfloat16)
        self.dw, self.db = z(C, 2), z(2)
        self.loss, self.wsum = z(1, v=acc), z(1, v=acc)
        self.prob_e, self.esums, self.hist = z(NPIX), z(5, v=acc), torch.full((2, 256), int(acc), dtype=torch.int64, device=hu.DEV)

    def train(self):
        return [("prob", self.prob), ("dact", self.dact), ("dw", self.dw), ("db", self.db), ("loss_sum", self.loss), ("weight_sum", self.wsum)]

    def eval(self):
        return [("prob (eval)", self.prob_e), ("eval sums", self.esums), ("hist", self.hist)]

    def all(self):
        return [("prob (sums pass)", self.prob_a), ("dice_sums", self.sums)] + self.train() + self.eval()


def _hbits(t):
    return t if t.dtype == torch.int64 else _bits(t)


class Dev:
    """one case's inputs on the device"""

    def __init__(self, C, act, w, b, labels, class_w, pixel_w):
        self.C = C
        self.act, self.w, self.b = hu.dev_bf16(act), hu.dev_f32(w), hu.dev_f32(b)
        self.lab = _dev_labels(labels)
        self.cw = hu.dev_f32(np.asarray(class_w, np.float32)) if class_w is not None else None
        self.pw = hu.dev_f32(pixel_w) if pixel_w is not None else None
        self.ws_t = torch.zeros(lib().rsu_head_dice_ws_floats(NPIX, C), dtype=torch.float32, device=hu.DEV)
        self.ws_e = torch.zeros(lib().rsu_head_eval_ws_floats(NPIX, C), dtype=torch.float32, device=hu.DEV)

    def head(self):
        return hu.ptr(self.act), hu.ptr(self.w), hu.ptr(self.b), hu.ptr(self.lab)


def _train(d, gamma, dice=False, o=None, entry="rsu_head_fwd_bwd_focal"):
    """the training entry (behind rsu_head_dice_sums with dice); entry: a sibling of rsu.h to run on the same inputs instead"""
    o = o or Out(d.C)
    p = hu.ptr
    if dice:
        call("rsu_head_dice_sums", *d.head(), p(d.pw), p(o.prob_a), p(o.sums), p(d.ws_t), NPIX, d.C, hu.stream())
    tail = (p(o.prob), p(o.loss), p(o.wsum), p(o.dact), p(o.dw), p(o.db), p(d.ws_t), NPIX, d.C, INV, hu.stream())
    if entry == "rsu_head_fwd_bwd_focal":
        call(entry, *d.head(), p(d.cw), p(d.pw), gamma, p(o.sums) if dice else None, LAM, SMOOTH, *tail)
    elif entry == "rsu_head_fwd_bwd_dice":
        call(entry, *d.head(), p(d.cw), p(d.pw), p(o.sums), LAM, SMOOTH, *tail)
    else:
        call("rsu_head_fwd_bwd_w", *d.head(), p(d.cw), p(d.pw), *tail)
    torch.cuda.synchronize()
    return o


def _eval(d, gamma, o=None, entry="rsu_head_eval_focal"):
    o = o or Out(d.C)
    p = hu.ptr
    tail = (p(o.prob_e), p(o.esums), p(o.hist), p(d.ws_e), NPIX, d.C, hu.stream())
    if entry == "rsu_head_eval_focal":
        call(entry, *d.head(), p(d.cw), p(d.pw), gamma, *tail)
    else:
        call("rsu_head_eval", *d.head(), p(d.cw), p(d.pw), *tail)
    torch.cuda.synchronize()
    return o


@functools.lru_cache(maxsize=None)
def _case(C, mode, scale=1.0):
    """inputs of a case, drawn once and never written: (act, w, b, labels, class_w, pixel_w, ignored mask)"""
    rng, act, w, b, labels = _inputs(C)
    w = (w * np.float32(scale)).astype(np.float32)
    class_w = CW if mode in ("class", "both", "ignored") else None
    pixel_w = _weight_map(rng) if mode in ("map", "both", "ignored") else None
    if mode == "ignored":
        labels, _ = _with_ignored(rng, labels)
    ign = (labels != 0) & (labels != 1)
    return act, w, b, labels, class_w, pixel_w, ign


@functools.lru_cache(maxsize=None)
def _ref(C, mode, gamma, dice, scale=1.0):
    """the float64 reference of a case, computed once and shared"""
    act, w, b, labels, class_w, pixel_w, ign = _case(C, mode, scale)
    safe_pw = None if pixel_w is None else np.where(ign, 1.0, pixel_w)
    return FU.Ref(act, w, b, labels, class_w, safe_pw, INV, gamma, lam=LAM if dice else 0.0)


def _check(o, ref, what, ign):
    got_loss, got_wsum = float(hu.host(o.loss)[0]), float(hu.host(o.wsum)[0])
    print("%s: loss/npix got %.9g ref %.9g; weight_sum got %.9g ref %.9g; max |dw| %.3g" % (what, got_loss / NPIX, ref.loss_sum / NPIX, got_wsum,
                                                                                         ref.wsum, float(np.abs(ref.dw).max())))
    for name, t in o.train():
        assert bool(torch.all(torch.isfinite(t.to(torch.float32)))), (what, name)
    hu.assert_f32_close(hu.host(o.prob), ref.prob, what + " prob", rtol=1e-4, atol_scale=1e-6)
    assert abs(got_loss / NPIX - ref.loss_sum / NPIX) < 2e-5 * max(1.0, abs(ref.loss_sum / NPIX)), (what, got_loss, ref.loss_sum)
    assert abs(got_loss - ref.loss_sum) <= 2e-5 * abs(ref.loss_sum), (what, got_loss, ref.loss_sum)
    assert abs(got_wsum - ref.wsum) <= 2e-5 * abs(ref.wsum), (what, got_wsum, ref.wsum)
    hu.assert_bf16_close(hu.host(o.dact), ref.dact, what + " dact")
    hu.assert_f32_close(hu.host(o.dw), ref.dw, what + " dw")
    hu.assert_f32_close(hu.host(o.db), ref.db, what + " db")
    rows = o.dact[torch.from_numpy(ign).to(hu.DEV)]
    assert rows.shape[0] == int(ign.sum()) and not torch.any(_bits(rows) != 0), "dact rows of ignored pixels must be exactly +0"


# ------------------------------------------------------------------------------------------- 1. the op against the reference
@pytest.mark.parametrize("dice", [False, True], ids=["focal", "focal+dice"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gamma", FU.GAMMAS)
@pytest.mark.parametrize("C", [64, 16])
def test_focal_head_against_float64_autograd(C, gamma, mode, dice):
    act, w, b, labels, class_w, pixel_w, ign = _case(C, mode)
    d = Dev(C, act, w, b, labels, class_w, pixel_w)
    o = _train(d, gamma, dice)
    ref = _ref(C, mode, gamma, dice)
    what = "focal head (C=%d, gamma=%g, %s%s)" % (C, gamma, mode, ", dice" if dice else "")
    _check(o, ref, what, ign)
    # the modulation is a real part of these gradients, not noise below the tolerance
    ce_only = _ref(C, mode, 0.0, dice)
    assert float(np.abs(ref.dw - ce_only.dw).max()) > 1e-2 * float(np.abs(ce_only.dw).max())
    # and the evaluation head on the same inputs: the same objective, the sums of the family
    e = _eval(d, gamma)
    hu.assert_f32_close(hu.host(e.esums), np.array([ref.loss_sum, ref.wsum, ref.sums[0], ref.sums[1], ref.sums[2]]), what + " eval sums", rtol=2e-5)
    hu.assert_f32_close(hu.host(e.prob_e), ref.prob, what + " eval prob", rtol=1e-4, atol_scale=1e-6)


# ------------------------------------------------------------------------------------------- 2. saturated logits
@pytest.mark.parametrize("dice", [False, True], ids=["focal", "focal+dice"])
@pytest.mark.parametrize("gamma", FU.GAMMAS)
@pytest.mark.parametrize("C", [64, 16])
def test_saturated_logits_stay_finite(C, gamma, dice):
    """w x 60: p_o == 0 at 154 / 680 pixels and p_t == 0 at 591 / 1355 (C = 16 / 64) in float32 (tests/test_focal_host.py counts them)"""
    act, w, b, labels, class_w, pixel_w, ign = _case(C, "ignored", FU.SATURATE)
    d = Dev(C, act, w, b, labels, class_w, pixel_w)
    o = _train(d, gamma, dice)
    what = "saturated focal head (C=%d, gamma=%g%s)" % (C, gamma, ", dice" if dice else "")
    p = o.prob[torch.from_numpy(~ign).to(hu.DEV)]
    assert int((p == 0).sum()) > 0 and int((p == 1).sum()) > 100, what          # (the corners are there on the device too)
    _check(o, _ref(C, "ignored", gamma, dice, FU.SATURATE), what, ign)
    e = _eval(d, gamma)
    for name, t in e.eval():
        assert bool(torch.all(torch.isfinite(t.to(torch.float32)))), (what, name)
    assert torch.equal(_bits(e.esums[:1]), _bits(o.loss)), what


# ------------------------------------------------------------------------------------------- 3. bit relations
@pytest.mark.parametrize("C", [64, 16])
def test_gamma_zero_launches_the_existing_heads(C):
    act, w, b, labels, class_w, pixel_w, _ = _case(C, "ignored")
    d = Dev(C, act, w, b, labels, class_w, pixel_w)
    for dice, sibling in ((False, "rsu_head_fwd_bwd_w"), (True, "rsu_head_fwd_bwd_dice")):
        got, ref = _train(d, 0.0, dice), _train(d, 0.0, dice, entry=sibling)
        assert float(ref.loss.item()) > 0
        for (name, t), (_, r) in zip(got.all()[:8], ref.all()[:8]):
            assert torch.equal(_bits(t), _bits(r)), (sibling, name)
    got, ref = _eval(d, 0.0), _eval(d, 0.0, entry="rsu_head_eval")
    for (name, t), (_, r) in zip(got.eval(), ref.eval()):
        assert torch.equal(_hbits(t), _hbits(r)), name
    assert int(ref.hist.sum()) == int(((labels == 0) | (labels == 1)).sum())


@pytest.mark.parametrize("gamma", FU.GAMMAS)
@pytest.mark.parametrize("C", [64, 16])
def test_bits_shared_with_the_family(C, gamma):
    act, w, b, labels, class_w, pixel_w, _ = _case(C, "ignored")
    d = Dev(C, act, w, b, labels, class_w, pixel_w)
    plain, focal, focal_d = _train(d, 0.0, entry="rsu_head_fwd_bwd_w"), _train(d, gamma), _train(d, gamma, dice=True)
    ev, ev_f = _eval(d, 0.0, entry="rsu_head_eval"), _eval(d, gamma)
    for o in (focal, focal_d):
        assert torch.equal(_bits(o.prob), _bits(plain.prob)) and torch.equal(_bits(o.wsum), _bits(plain.wsum))
        assert not torch.equal(_bits(o.loss), _bits(plain.loss)) and float(o.loss.item()) < float(plain.loss.item())
    assert torch.equal(_bits(focal_d.loss), _bits(focal.loss)), "the Dice term does not enter loss_sum"
    assert torch.equal(_bits(focal_d.prob_a), _bits(plain.prob))
    assert torch.equal(_bits(ev_f.prob_e), _bits(plain.prob))
    assert torch.equal(_bits(ev_f.esums[:1]), _bits(focal.loss)), "evaluation sums[0] from zero == training loss_sum"
    assert torch.equal(_bits(ev_f.esums[1:]), _bits(ev.esums[1:])) and torch.equal(ev_f.hist, ev.hist)
    assert torch.equal(_bits(ev_f.esums[1:2]), _bits(plain.wsum))
    # two runs give the same bits
    again, again_d, again_e = _train(d, gamma), _train(d, gamma, dice=True), _eval(d, gamma)
    for a, c in ((focal, again), (focal_d, again_d), (ev_f, again_e)):
        for (name, t), (_, r) in zip(a.all(), c.all()):
            assert torch.equal(_hbits(t), _hbits(r)), name
    # the accumulators accumulate: a second evaluation on top of the first doubles the counts
    twice = _eval(d, gamma, o=_eval(d, gamma))
    assert torch.equal(twice.hist, 2 * ev_f.hist) and float(twice.esums[1].item()) == 2.0 * float(ev_f.esums[1].item())


@pytest.mark.parametrize("dice", [False, True], ids=["focal", "focal+dice"])
@pytest.mark.parametrize("C", [64, 16])
def test_ignored_pixels_carry_nothing(C, dice):
    """test_gpu_weighted_loss.test_ignored_labels' check: other junk in pixel_w at ignored pixels and other ignored label values"""
    rng = np.random.RandomState(C + 1)
    act, w, b, labels, class_w, pixel_w, ign = _case(C, "ignored")
    o = _train(Dev(C, act, w, b, labels, class_w, pixel_w), 2.0, dice)
    e = _eval(Dev(C, act, w, b, labels, class_w, pixel_w), 2.0)
    labels2, pixel_w2 = labels.copy(), pixel_w.copy()
    labels2[ign] = np.where(labels[ign] == -1, 7, -(2 ** 40))
    pixel_w2[ign] = (3.0 + 100.0 * rng.rand(int(ign.sum()))).astype(np.float32)
    pixel_w2[np.nonzero(ign)[0][:3]] = [np.inf, np.nan, -1e30]
    d2 = Dev(C, act, w, b, labels2, class_w, pixel_w2)
    o2, e2 = _train(d2, 2.0, dice), _eval(d2, 2.0)
    for (name, t), (_, t2) in zip(o.all()[:8] + e.eval(), o2.all()[:8] + e2.eval()):
        assert torch.equal(_hbits(t), _hbits(t2)), name
    assert bool(torch.all(torch.isfinite(o2.dw))) and bool(torch.all(torch.isfinite(e2.esums)))


# ------------------------------------------------------------------------------------------- 4. argument errors
def test_argument_errors_write_nothing():
    C = 16
    act, w, b, labels, class_w, pixel_w, _ = _case(C, "ignored")
    d = Dev(C, act, w, b, labels, class_w, pixel_w)
    d.ws_t.fill_(7.0)
    d.ws_e.fill_(7.0)
    o = Out(C, fill=7.0, acc=7.0)
    L, p, st = lib(), hu.ptr, hu.stream()

    def train(gamma=2.0, dice_sums=o.sums, lam=LAM, smooth=SMOOTH, C=C, npix=NPIX, **null):
        a = dict(act=d.act, w=d.w, b=d.b, labels=d.lab, prob=o.prob, loss=o.loss, dact=o.dact, dw=o.dw, db=o.db, ws=d.ws_t)
        a.update(null)
        return L.rsu_head_fwd_bwd_focal(p(a["act"]), p(a["w"]), p(a["b"]), p(a["labels"]), p(d.cw), p(d.pw), gamma, p(dice_sums), lam, smooth,
                                        p(a["prob"]), p(a["loss"]), p(o.wsum), p(a["dact"]), p(a["dw"]), p(a["db"]), p(a["ws"]), npix, C, INV, st)

    def evaluate(gamma=2.0, C=C, npix=NPIX, **null):
        a = dict(act=d.act, w=d.w, b=d.b, labels=d.lab, prob=o.prob_e, sums=o.esums, hist=o.hist, ws=d.ws_e)
        a.update(null)
        return L.rsu_head_eval_focal(p(a["act"]), p(a["w"]), p(a["b"]), p(a["labels"]), p(d.cw), p(d.pw), gamma, p(a["prob"]), p(a["sums"]),
                                     p(a["hist"]), p(a["ws"]), npix, C, st)
    for fn in (train, evaluate):
        for gamma in (-1.0, -1e-6, float("nan"), float("inf"), -float("inf")):
            assert fn(gamma=gamma) == RSU_EINVAL, (fn.__name__, gamma)
        for bad_c in (0, 12, 24, 520):
            assert fn(C=bad_c) == RSU_EINVAL, (fn.__name__, bad_c)
        assert fn(npix=0) == RSU_EINVAL and fn(npix=-5) == RSU_EINVAL
        assert fn(gamma=0.0, npix=0) == RSU_EINVAL and fn(gamma=0.0, labels=None) == RSU_EINVAL      # (gamma = 0 refuses the same)
    for name in ("act", "w", "b", "labels", "prob", "loss", "dact", "dw", "db", "ws"):
        assert train(**{name: None}) == RSU_EINVAL, name
        assert train(dice_sums=None, **{name: None}) == RSU_EINVAL, name
    for name in ("act", "w", "b", "labels", "prob", "sums", "hist", "ws"):
        assert evaluate(**{name: None}) == RSU_EINVAL, name
    # the Dice argument rules, with dice_sums given
    for kw in (dict(smooth=0.0), dict(smooth=-1.0), dict(smooth=float("nan")), dict(smooth=float("inf")), dict(lam=-0.5), dict(lam=float("nan")),
               dict(lam=float("inf"))):
        assert train(**kw) == RSU_EINVAL, kw
        assert train(gamma=0.0, **kw) == RSU_EINVAL, kw
    torch.cuda.synchronize()
    for name, t in o.all() + [("ws (training)", d.ws_t), ("ws (evaluation)", d.ws_e)]:
        assert bool(torch.all(t == 7)), "%s was written by a refused call" % name
    # without dice_sums, dice_scale and smooth are not looked at
    ok = Out(C)
    assert L.rsu_head_fwd_bwd_focal(*d.head(), p(d.cw), p(d.pw), 2.0, None, float("nan"), -1.0, p(ok.prob), p(ok.loss), p(ok.wsum), p(ok.dact),
                                    p(ok.dw), p(ok.db), p(d.ws_t), NPIX, C, INV, st) == 0
    assert torch.equal(_bits(ok.loss), _bits(_train(d, 2.0).loss)) and torch.equal(_bits(ok.dact), _bits(_train(d, 2.0).dact))


# ------------------------------------------------------------------------------------------- 5. rounding of dact
@pytest.mark.parametrize("C", [64, 16])
def test_dact_is_rounded_once(C):
    """hiputil.assert_bf16_rounded on the unscaled inputs only (tests/test_focal_host.py: the float32 restatement alone leaves 3e-5 to 1e-4
    of the elements off the reference's bits here; on the saturated inputs gamma amplifies the fp32 noise of the logits in elements far
    below the absolute tolerance, so that case gets assert_bf16_close only)"""
    act, w, b, labels, class_w, pixel_w, _ = _case(C, "both")
    o = _train(Dev(C, act, w, b, labels, class_w, pixel_w), 2.0)
    mismatch, bias, n = hu.assert_bf16_rounded(hu.host(o.dact), _ref(C, "both", 2.0, False).dact, "focal dact C=%d" % C)
    print("focal dact C=%d: mismatch %.2e bias %+.4f ulp over %d elements" % (C, mismatch, bias, n))


# ------------------------------------------------------------------------------------------- 6. the network
def _op_on_net(m, gamma, dice_scale):
    """the op-level call on the activations a net's pass left behind, with the net's own weights, labels and pixel weights"""
    C, npix = m.root, m.B * m.P * m.P
    p = hu.ptr
    z = lambda *s, dtype=torch.float32: torch.zeros(s, dtype=dtype, device=hu.DEV)  # noqa: E731
    prob, dact, dw, db, loss, wsum, sums = z(npix), z(npix, C, dtype=torch.bfloat16), z(C, 2), z(2), z(1), z(1), z(3)
    ws = z(lib().rsu_head_dice_ws_floats(npix, C))
    head = (p(m.act[m.last_name]), p(m.w["weight_output/kernel"]), p(m.w["weight_output/bias"]), p(m.labels))
    pw = m.border_map if m.border_weight > 0 else m.pixel_weights
    if dice_scale > 0:
        call("rsu_head_dice_sums", *head, p(pw), p(prob), p(sums), p(ws), npix, C, hu.stream())
    call("rsu_head_fwd_bwd_focal", *head, p(m._class_w_dev), p(pw), gamma, p(sums) if dice_scale > 0 else None, dice_scale, m.dice_smooth, p(prob),
         p(loss), p(wsum), p(dact), p(dw), p(db), p(ws), npix, C, 1.0 / npix, hu.stream())
    torch.cuda.synchronize()
    return prob, dact, dw, db, loss, wsum


@pytest.mark.parametrize("L,root,dilated,P", NETS)
def test_net_gamma_zero_is_the_default_net(L, root, dilated, P):
    a, b = _net(L, root, dilated, P, None), _net(L, root, dilated, P, None, focal_gamma=0)
    assert b.focal_gamma == 0.0
    _batch(a)
    _batch(b)
    ga, pa, la, _, _ = _step(a)
    gb, pb, lb, _, _ = _step(b)
    assert torch.equal(_bits(ga), _bits(gb)) and torch.equal(_bits(pa), _bits(pb)) and torch.equal(_bits(la), _bits(lb))
    assert float(la.item()) > 0 and bool(torch.any(ga != 0))
    with pytest.raises(RsuError):
        b.focal_gamma = -1.0
    with pytest.raises(RsuError):
        _net(L, root, dilated, P, None, focal_gamma=float("nan"))


@pytest.mark.parametrize("kw", [dict(), dict(dice_weight=LAM), dict(border_weight=3.0), dict(dice_weight=LAM, border_weight=3.0)], ids=str)
@pytest.mark.parametrize("L,root,dilated,P", NETS)
def test_net_dispatches_to_the_focal_head(L, root, dilated, P, kw):
    """the head's outputs inside the net are the op-level call's on the same activations, bit for bit; everything behind the head is
    unchanged code"""
    m = _net(L, root, dilated, P, CW, focal_gamma=2.0, **kw)
    _batch(m)
    m.labels[0, :2] = -1
    gen = torch.Generator(device="cpu").manual_seed(3)
    m.set_pixel_weights(0.25 + torch.rand((2, P, P), generator=gen))
    _, prob, loss, wsum, _ = _step(m)
    rprob, rdact, rdw, rdb, rloss, rwsum = _op_on_net(m, 2.0, m.dice_weight)
    assert float(loss.item()) > 0 and float(wsum.item()) > 0
    assert torch.equal(_bits(prob.reshape(-1)), _bits(rprob)) and torch.equal(_bits(loss), _bits(rloss)) and torch.equal(_bits(wsum), _bits(rwsum))
    assert torch.equal(_bits(m.grad[m.last_name].reshape(-1, root)), _bits(rdact))
    assert torch.equal(_bits(m.g["weight_output/kernel"].reshape(-1)), _bits(rdw.reshape(-1)))
    assert torch.equal(_bits(m.g["weight_output/bias"]), _bits(rdb))
    # and it is not the cross-entropy head's result
    plain = _net(L, root, dilated, P, CW, **kw)
    _batch(plain)
    plain.labels[0, :2] = -1
    plain.set_pixel_weights(m.pixel_weights)
    _, pprob, ploss, pwsum, _ = _step(plain)
    assert torch.equal(_bits(pprob), _bits(prob)) and torch.equal(_bits(pwsum), _bits(wsum)) and float(loss.item()) < float(ploss.item())
    assert bool(torch.all(torch.isfinite(m.flat_g))) and not torch.equal(m.flat_g, plain.flat_g)


@pytest.mark.parametrize("L,root,dilated,P", NETS)
def test_net_evaluates_the_objective_it_trains_on(L, root, dilated, P):
    m = _net(L, root, dilated, P, CW, focal_gamma=2.0)
    _batch(m)
    m.labels[1, :3] = -1
    m.reset_eval()
    m.forward_device(keep=1.0)
    m.evaluate_device()
    torch.cuda.synchronize()
    sums, hist = m.eval_sums.clone(), m.eval_hist.clone()
    _, _, _, _, rloss, rwsum = _op_on_net(m, 2.0, 0.0)
    assert torch.equal(_bits(sums[:1]), _bits(rloss)) and torch.equal(_bits(sums[1:2]), _bits(rwsum)) and float(rloss.item()) > 0
    assert int(hist.sum()) == int(((m.labels == 0) | (m.labels == 1)).sum())
    # a net without gamma scores the cross-entropy on the same activations: the same counts, a larger first sum
    plain = _net(L, root, dilated, P, CW)
    _batch(plain)
    plain.labels[1, :3] = -1
    plain.reset_eval()
    plain.forward_device(keep=1.0)
    plain.evaluate_device()
    torch.cuda.synchronize()
    assert torch.equal(plain.eval_hist, hist) and torch.equal(_bits(plain.eval_sums[1:]), _bits(sums[1:]))
    assert float(plain.eval_sums[0].item()) > float(sums[0].item())


# ------------------------------------------------------------------------------------------- the model
def test_model_trains_evaluates_and_checkpoints_with_focal_gamma(tmp_path):
    m = _model(focal_gamma=2.0, class_weights="1,3")
    assert m.net.focal_gamma == 2.0
    rng = np.random.RandomState(2)
    S, P = m.input_size, 20
    for _ in range(3):
        X = rng.rand(2, S, S, 3).astype(np.float32)
        y = (rng.rand(2, P, P) < 0.3).astype(np.int64)
        loss, _ = m.train_step(X, y)
        assert np.isfinite(float(loss)) and float(loss) > 0
    assert bool(torch.all(torch.isfinite(m.net.flat_w)))
    # evaluate()'s loss is focal_loss_terms of the probabilities the same weights predict
    X = rng.rand(4, S, S, 3).astype(np.float32)
    y = (rng.rand(4, P, P) < 0.3).astype(np.int64)
    y[0, :4] = -1
    v = m.evaluate(X, y)
    probs = []
    for t0 in (0, 2):
        m.net.x.copy_(torch.from_numpy(X[t0:t0 + 2]))
        m.net.forward_device(keep=1.0)
        m.net.labels.copy_(torch.from_numpy(y[t0:t0 + 2]))
        m.net.reset_eval()
        m.net.evaluate_device()
        torch.cuda.synchronize()
        probs.append(m.net.prob.cpu().numpy().reshape(2, P, P))
    ref_loss, ref_wsum = focal_loss_terms(np.concatenate(probs), y, 2.0, (1.0, 3.0))
    print("evaluate: loss %.9g, focal_loss_terms / pixels %.9g" % (v["loss"], ref_loss / y.size))
    assert abs(v["loss"] - ref_loss / y.size) <= 2e-5 * ref_loss / y.size
    assert abs(float(v["sums"][1]) - ref_wsum) <= 2e-5 * ref_wsum
    assert v["objective"] == v["loss"]          # (no Dice term in this model)
    # a checkpoint round trip needs no new variable, and the restored model resumes with the same bits
    sd = m.net.state_dict()
    plain = _model(class_weights="1,3")
    assert sorted(sd) == sorted(plain.net.state_dict()) and not [n for n in sd if "focal" in n.lower()]
    path = m.save_as(str(tmp_path / "ck" / "model.chkpt"))
    X = rng.rand(2, S, S, 3).astype(np.float32)
    y = (rng.rand(2, P, P) < 0.3).astype(np.int64)
    la, _ = m.train_step(X, y)
    b = _model(focal_gamma=2.0, class_weights="1,3")
    b.restore(file=path)
    lb, _ = b.train_step(X, y)
    torch.cuda.synchronize()
    assert float(la) == float(lb) and torch.equal(_bits(m.net.flat_w), _bits(b.net.flat_w))
