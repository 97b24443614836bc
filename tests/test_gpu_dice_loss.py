"""-m gpu: the soft-Dice head (rsu.h rsu_head_dice_sums + rsu_head_fwd_bwd_dice) through the C ABI against float64 torch autograd built here
from the same bf16-rounded inputs, the device buffer between the two launches, and the network / model level above it. Inputs are
tests/test_gpu_ops.py::test_head's; tolerances are the hiputil defaults as tests/test_gpu_weighted_loss.py uses them, 2e-5 relative for
scalar sums (as for weight_sum there)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import hiputil as hu  # noqa: E402
from tests.head_util import (LAM, NETS, NPIX, RSU_EINVAL, SMOOTH, Ref, _batch, _bits, _dev_labels, _inputs, _model, _net, _step,  # noqa: E402
                             _weight_map, _with_ignored)
from road_segmentation_unet_amd._lib import RsuError, call, lib  # noqa: E402
from road_segmentation_unet_amd.model import dice_from_sums  # noqa: E402



class Out:
    def __init__(self, C, npix=NPIX, fill=0.0):
        z = lambda *s, dtype=torch.float32: torch.full(s, fill, dtype=dtype, device=hu.DEV)  # noqa: E731
        self.prob_a, self.sums = z(npix), z(3)
        self.prob, self.dact = z(npix), z(npix, C, dtype=torch.bfloat16)
        self.dw, self.db = z(C, 2), z(2)
        self.loss, self.wsum = z(1), z(1)

    def all(self):
        return [("prob (sums pass)", self.prob_a), ("dice_sums", self.sums), ("prob", self.prob), ("dact", self.dact), ("dw", self.dw),
                ("db", self.db), ("loss_sum", self.loss), ("weight_sum", self.wsum)]


def _run(C, act_d, w_d, b_d, labels, class_w, pixel_w, inv, lam=LAM, smooth=SMOOTH, sums=None, npix=NPIX):
    """the two calls on one stream, nothing between them; sums: a hand-written {I, P, Y} for the second call instead of the first's"""
    o = Out(C, npix)
    ws = torch.zeros(lib().rsu_head_dice_ws_floats(npix, C), dtype=torch.float32, device=hu.DEV)
    lab = labels if torch.is_tensor(labels) else _dev_labels(labels)
    cw = hu.dev_f32(np.asarray(class_w, np.float32)) if class_w is not None else None
    pw = pixel_w if (pixel_w is None or torch.is_tensor(pixel_w)) else hu.dev_f32(pixel_w)
    call("rsu_head_dice_sums", hu.ptr(act_d), hu.ptr(w_d), hu.ptr(b_d), hu.ptr(lab), hu.ptr(pw), hu.ptr(o.prob_a), hu.ptr(o.sums), hu.ptr(ws),
         npix, C, hu.stream())
    given = o.sums if sums is None else hu.dev_f32(np.asarray(sums, np.float32))
    call("rsu_head_fwd_bwd_dice", hu.ptr(act_d), hu.ptr(w_d), hu.ptr(b_d), hu.ptr(lab), hu.ptr(cw), hu.ptr(pw), hu.ptr(given), lam, smooth,
         hu.ptr(o.prob), hu.ptr(o.loss), hu.ptr(o.wsum), hu.ptr(o.dact), hu.ptr(o.dw), hu.ptr(o.db), hu.ptr(ws), npix, C, inv, hu.stream())
    torch.cuda.synchronize()
    return o


def _check_sums(o, ref, what):
    got = hu.host(o.sums).astype(np.float64)
    print("%s: I P Y got %s ref %s" % (what, got, ref.sums))
    for g, r, n in zip(got, ref.sums, "IPY"):
        assert r > 1.0, (what, n, r)                      # (no sum is near zero: the relative bound means something)
        assert abs(g - r) <= 2e-5 * abs(r), (what, n, g, r)
    hu.assert_f32_close(hu.host(o.prob_a), ref.prob, what + " prob (sums pass)", rtol=1e-4, atol_scale=1e-6)


def _check_grads(o, ref, what, npix=NPIX):
    got_loss, got_wsum = float(hu.host(o.loss)[0]), float(hu.host(o.wsum)[0])
    print("%s: loss/npix got %.9g ref %.9g; weight_sum got %.9g ref %.9g; max |dw| %.3g" % (what, got_loss / npix, ref.ce_sum / npix, got_wsum,
                                                                                         ref.wsum, float(np.abs(ref.dw).max())))
    hu.assert_f32_close(hu.host(o.prob), ref.prob, what + " prob", rtol=1e-4, atol_scale=1e-6)
    assert abs(got_loss / npix - ref.ce_sum / npix) < 2e-5 * max(1.0, abs(ref.ce_sum / npix)), (what, got_loss, ref.ce_sum)
    assert abs(got_wsum - ref.wsum) <= 2e-5 * abs(ref.wsum), (what, got_wsum, ref.wsum)
    hu.assert_bf16_close(hu.host(o.dact), ref.dact, what + " dact")
    hu.assert_f32_close(hu.host(o.dw), ref.dw, what + " dw")
    hu.assert_f32_close(hu.host(o.db), ref.db, what + " db")
    rows = o.dact[torch.from_numpy(~ref.valid).to(hu.DEV)]
    assert rows.shape[0] == int((~ref.valid).sum()) and not torch.any(_bits(rows) != 0), "dact rows of ignored pixels must be exactly +0"


def _case(C, mode):
    rng, act, w, b, labels = _inputs(C)
    pixel_w = _weight_map(rng) if mode in ("map", "ignored") else None
    if pixel_w is not None:
        assert (pixel_w == 0).sum() > 0
    if mode == "ignored":
        labels, _ = _with_ignored(rng, labels)
    return rng, act, w, b, labels, pixel_w


# ------------------------------------------------------------------------------------------- the op
@pytest.mark.parametrize("C", [64, 16])
@pytest.mark.parametrize("mode", ["plain", "map", "ignored"])
def test_dice_sums_against_reference(C, mode):
    _, act, w, b, labels, pixel_w = _case(C, mode)
    inv = 1.0 / (2 * NPIX)
    o = _run(C, hu.dev_bf16(act), hu.dev_f32(w), hu.dev_f32(b), labels, None, pixel_w, inv)
    _check_sums(o, Ref(act, w, b, labels, None, pixel_w, inv), "dice sums (%s, C=%d)" % (mode, C))
    assert torch.equal(_bits(o.prob), _bits(o.prob_a)), "both passes write the same prob bits"


@pytest.mark.parametrize("C", [64, 16])
@pytest.mark.parametrize("mode,class_w", [("plain", None), ("plain", (0.6, 2.5)), ("ignored", (0.6, 2.5)), ("ignored", None)])
def test_dice_gradients_against_float64_autograd(C, mode, class_w):
    _, act, w, b, labels, pixel_w = _case(C, mode)
    inv = 1.0 / (2 * NPIX)
    o = _run(C, hu.dev_bf16(act), hu.dev_f32(w), hu.dev_f32(b), labels, class_w, pixel_w, inv)
    ref = Ref(act, w, b, labels, class_w, pixel_w, inv)
    _check_grads(o, ref, "dice head (%s, class_w %s, C=%d)" % (mode, class_w, C))
    # the Dice term is a real part of these gradients, not noise below the tolerance: without it the same check fails
    ce_only = Ref(act, w, b, labels, class_w, pixel_w, inv, lam=0.0)
    assert float(np.abs(ref.dw - ce_only.dw).max()) > 1e-2 * float(np.abs(ref.dw).max())


@pytest.mark.parametrize("C", [64, 16])
def test_second_pass_reads_the_buffer(C):
    """hand-written sums that differ from the batch's own: the outputs follow the buffer (nothing is recomputed in pass B)"""
    _, act, w, b, labels, pixel_w = _case(C, "ignored")
    inv = 1.0 / (2 * NPIX)
    own = Ref(act, w, b, labels, (0.6, 2.5), pixel_w, inv)
    given = [0.25 * own.sums[0], 3.0 * own.sums[1] + 11.0, 0.5 * own.sums[2]]
    o = _run(C, hu.dev_bf16(act), hu.dev_f32(w), hu.dev_f32(b), labels, (0.6, 2.5), pixel_w, inv, sums=given)
    ref = Ref(act, w, b, labels, (0.6, 2.5), pixel_w, inv, sums=[float(np.float32(v)) for v in given])
    _check_grads(o, ref, "dice head on given sums (C=%d)" % C)
    assert float(np.abs(ref.dw - own.dw).max()) > 1e-2 * float(np.abs(own.dw).max())   # (the two references are far apart)
    _check_sums(o, own, "sums of the same run (C=%d)" % C)                              # pass A still reported the batch's own


@pytest.mark.parametrize("C", [64, 16])
def test_ignored_pixels_carry_nothing(C):
    rng, act, w, b, labels, pixel_w = _case(C, "ignored")
    ign = (labels != 0) & (labels != 1)
    ad, wd, bd = hu.dev_bf16(act), hu.dev_f32(w), hu.dev_f32(b)
    inv = 1.0 / (2 * NPIX)
    o = _run(C, ad, wd, bd, labels, (0.6, 2.5), pixel_w, inv)
    labels2, pixel_w2 = labels.copy(), pixel_w.copy()
    labels2[ign] = np.where(labels[ign] == -1, 7, -(2 ** 40))
    pixel_w2[ign] = (3.0 + 100.0 * rng.rand(int(ign.sum()))).astype(np.float32)
    pixel_w2[np.nonzero(ign)[0][:3]] = [np.inf, np.nan, -1e30]
    o2 = _run(C, ad, wd, bd, labels2, (0.6, 2.5), pixel_w2, inv)
    for (name, t), (_, t2) in zip(o.all(), o2.all()):
        assert torch.equal(_bits(t), _bits(t2)), name
    assert bool(torch.all(torch.isfinite(o2.sums))) and bool(torch.all(torch.isfinite(o2.dw)))


@pytest.mark.parametrize("C,npix", [(64, NPIX), (16, NPIX), (64, 4 * 388 * 388)])
def test_dice_head_is_deterministic(C, npix):
    gen = torch.Generator(device="cpu").manual_seed(C + npix)
    if npix == NPIX:
        rng, act, w, b, labels, pixel_w = _case(C, "ignored")
        ad, wd, bd, lab, pw = hu.dev_bf16(act), hu.dev_f32(w), hu.dev_f32(b), _dev_labels(labels), hu.dev_f32(pixel_w)
    else:   # the c2 head geometry
        ad = torch.relu(torch.randn((npix, C), generator=gen)).to(hu.DEV).to(torch.bfloat16)
        wd, bd = (0.3 * torch.randn((C, 2), generator=gen)).to(hu.DEV), (0.1 * torch.randn(2, generator=gen)).to(hu.DEV)
        lab = (torch.rand(npix, generator=gen) < 0.2).to(torch.int64)
        lab[torch.rand(npix, generator=gen) < 0.05] = -1
        lab = lab.to(hu.DEV)
        pw = (0.25 + torch.rand(npix, generator=gen)).to(hu.DEV)
    first = _run(C, ad, wd, bd, lab, (0.6, 2.5), pw, 1.0 / npix, npix=npix)
    second = _run(C, ad, wd, bd, lab, (0.6, 2.5), pw, 1.0 / npix, npix=npix)
    for (name, t), (_, t2) in zip(first.all(), second.all()):
        assert torch.equal(_bits(t), _bits(t2)), name
    s = first.sums.cpu().numpy()
    print("npix %d C %d: I P Y %s, D %.6f" % (npix, C, s, dice_from_sums(s[0], s[1], s[2], SMOOTH)))
    assert bool(torch.all(first.sums > 0)) and bool(torch.any(first.dw != 0)) and bool(torch.all(torch.isfinite(first.dw)))


def test_dice_head_argument_checks():
    C = 16
    _, act, w, b, labels = _inputs(C)
    ad, wd, bd = hu.dev_bf16(act), hu.dev_f32(w), hu.dev_f32(b)
    lab = _dev_labels(labels)
    o = Out(C, fill=7.0)
    sums_in = torch.full((3,), 7.0, dtype=torch.float32, device=hu.DEV)
    n = lib().rsu_head_dice_ws_floats(NPIX, C)
    assert n >= lib().rsu_head_w_ws_floats(NPIX, C)
    ws = torch.full((n,), 7.0, dtype=torch.float32, device=hu.DEV)

    def rc_a(act=ad, w=wd, b=bd, labels=lab, prob=o.prob_a, sums=o.sums, ws=ws, C=C, npix=NPIX):
        return lib().rsu_head_dice_sums(hu.ptr(act), hu.ptr(w), hu.ptr(b), hu.ptr(labels), None, hu.ptr(prob), hu.ptr(sums), hu.ptr(ws), npix, C,
                                        hu.stream())

    def rc_b(act=ad, w=wd, b=bd, labels=lab, sums=sums_in, lam=LAM, smooth=SMOOTH, prob=o.prob, loss=o.loss, dact=o.dact, dw=o.dw, db=o.db,
             ws=ws, C=C, npix=NPIX):
        return lib().rsu_head_fwd_bwd_dice(hu.ptr(act), hu.ptr(w), hu.ptr(b), hu.ptr(labels), None, None, hu.ptr(sums), lam, smooth, hu.ptr(prob),
                                           hu.ptr(loss), hu.ptr(o.wsum), hu.ptr(dact), hu.ptr(dw), hu.ptr(db), hu.ptr(ws), npix, C,
                                           0.5 / NPIX, hu.stream())
    for rc in (rc_a, rc_b):
        for name in ("act", "w", "b", "labels", "prob", "sums", "ws"):
            assert rc(**{name: None}) == RSU_EINVAL, (rc.__name__, name)
        for bad_c in (0, 12, 24, 520):
            assert rc(C=bad_c) == RSU_EINVAL, (rc.__name__, bad_c)
        assert rc(npix=0) == RSU_EINVAL and rc(npix=-5) == RSU_EINVAL
    for name in ("loss", "dact", "dw", "db"):
        assert rc_b(**{name: None}) == RSU_EINVAL, name
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        assert rc_b(smooth=bad) == RSU_EINVAL, ("smooth", bad)
    for bad in (-0.5, float("nan"), float("inf"), -float("inf")):
        assert rc_b(lam=bad) == RSU_EINVAL, ("dice_scale", bad)
    torch.cuda.synchronize()
    for name, t in o.all() + [("ws", ws), ("dice_sums (input)", sums_in)]:
        assert bool(torch.all(t == 7.0)), "%s was written by a refused call" % name
    assert rc_b(lam=0.0) == 0      # dice_scale == 0 is allowed: the weighted cross-entropy alone
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- the network
@pytest.mark.parametrize("L,root,dilated,P", NETS)
def test_net_dice_weight_zero_is_the_default_net(L, root, dilated, P):
    a, b = _net(L, root, dilated, P), _net(L, root, dilated, P, dice_weight=0.0, dice_smooth=3.0)
    assert a.dice_weight == 0.0 and a.dice_smooth == 1.0 and tuple(a.dice_sums.shape) == (3,) and a.dice_sums.dtype == torch.float32
    _batch(a)
    _batch(b)
    ga, pa, la, _, sa = _step(a)
    gb, pb, lb, _, sb = _step(b)
    assert torch.equal(_bits(ga), _bits(gb)) and torch.equal(_bits(pa), _bits(pb)) and torch.equal(_bits(la), _bits(lb))
    assert float(la.item()) > 0 and bool(torch.any(ga != 0))
    assert not bool(torch.any(sa != 0)) and not bool(torch.any(sb != 0))     # no Dice launch ran
    # an explicit dice_scale=0 on a net that has a Dice weight: the same pass again
    b.dice_weight = 0.7
    gc, pc, lc, _, _ = _step(b, dice_scale=0.0)
    assert torch.equal(_bits(ga), _bits(gc)) and torch.equal(_bits(pa), _bits(pc)) and torch.equal(_bits(la), _bits(lc))


@pytest.mark.parametrize("L,root,dilated,P", NETS)
def test_net_dice_head_equals_the_standalone_op(L, root, dilated, P):
    cw = (0.6, 2.5)
    m = _net(L, root, dilated, P, class_weights=cw, dice_weight=LAM, dice_smooth=2.0)
    plain = _net(L, root, dilated, P, class_weights=cw)
    _batch(m)
    _batch(plain)
    gen = torch.Generator(device="cpu").manual_seed(3)
    wmap = 0.25 + torch.rand((2, P, P), generator=gen)
    for net in (m, plain):
        net.set_pixel_weights(wmap)
        net.labels[0, :3] = -1
    m.tune()
    assert m.dice_weight == LAM and m.dice_smooth == 2.0 and m.pixel_weights is not None and torch.equal(m.pixel_weights.cpu(), wmap)
    assert int((m.labels == -1).sum()) == 3 * P
    first = _step(m)
    second = _step(m)
    for x, y in zip(first, second):
        assert torch.equal(_bits(x), _bits(y))
    npix, C = m.B * P * P, root
    o = _run(C, m.act[m.last_name], m.w["weight_output/kernel"], m.w["weight_output/bias"], m.labels, cw, m.pixel_weights, 1.0 / npix, lam=LAM,
             smooth=2.0, npix=npix)
    for name, got, want in (("dw", m.g["weight_output/kernel"], o.dw), ("db", m.g["weight_output/bias"], o.db),
                            ("dact", m.grad[m.last_name], o.dact), ("prob", m.prob, o.prob),
                            ("loss_sum", m.loss_sum, o.loss), ("weight_sum", m.weight_sum, o.wsum), ("dice_sums", m.dice_sums, o.sums)):
        assert torch.equal(_bits(got.reshape(want.shape)), _bits(want)), name
    # and the term reaches the whole network: every other gradient differs from the cross-entropy-only net's
    gp = _step(plain)[0]
    assert torch.equal(_bits(first[1]), _bits(_step(plain)[1]))          # (same forward pass)
    n = m.n_live
    assert float((first[0][:n] - gp[:n]).abs().max()) > 1e-3 * float(gp[:n].abs().max())


def test_net_refuses_bad_dice_values():
    L, root, dilated, P = NETS[1]
    for kw in (dict(dice_weight=-0.1), dict(dice_weight=float("nan")), dict(dice_weight=float("inf")), dict(dice_weight="x"),
               dict(dice_smooth=0.0), dict(dice_smooth=-1.0), dict(dice_smooth=float("nan"))):
        with pytest.raises(RsuError):
            _net(L, root, dilated, P, **kw)
    m = _net(L, root, dilated, P, dice_weight=0.5)
    with pytest.raises(RsuError):
        m.dice_weight = -1.0
    with pytest.raises(RsuError):
        m.dice_smooth = 0.0
    assert m.dice_weight == 0.5 and m.dice_smooth == 1.0
    _batch(m)
    m.forward_device()
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(RsuError):
            m.backward_device(1.0 / (m.B * P * P), dice_scale=bad)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- the model
def _host_loss(prob, y, lam, smooth):
    p = np.asarray(prob, np.float64).reshape(-1)
    y = np.asarray(y, np.float64).reshape(-1)
    ce = -np.where(y > 0, np.log(p), np.log1p(-p)).mean()
    D = float(dice_from_sums(np.sum(p * y), np.sum(p), np.sum(y), smooth))
    return ce + lam * (1.0 - D), D


def test_model_trains_with_the_dice_term():
    """30 steps on one fixed batch. The batch is learnable and balanced: diagonal stripes 5 pixels wide, bright in the red channel where the
    label is 1 (noise elsewhere), half of the pixels each -- at balanced classes the cross-entropy does not pull the mean prediction away
    from 0.5, so D moves only by what the network learns about the stripes, which both terms reward."""
    lam = 1.0
    m = _model(dice_weight=lam)
    assert m.net.dice_weight == lam and m.net.dice_smooth == 1.0
    rng = np.random.RandomState(2)
    S, P = m.input_size, 20
    ii, jj = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    stripes = (((ii + jj) // 5) % 2).astype(np.float32)
    X = rng.rand(2, S, S, 3).astype(np.float32)
    X[1] = X[1, ::-1]
    masks = np.stack([stripes, stripes[::-1]])
    X[..., 0] = 0.1 + 0.8 * masks + 0.1 * X[..., 0]
    off = (S - P) // 2
    y = masks[:, off:off + P, off:off + P].astype(np.int64)
    assert 0.4 < y.mean() < 0.6
    w0 = m.net.flat_w.clone()
    Ds = []
    for step in range(30):
        loss, prob = m.train_step(X, y)
        ref, D = _host_loss(prob.cpu().numpy(), y, lam, 1.0)
        got = float(loss)
        Ds.append(D)
        print("step %2d: loss %.7f host %.7f  D %.5f" % (step, got, ref, D))
        assert abs(got - ref) <= 1e-5 * max(1.0, abs(ref)), (step, got, ref)
        s = m.net.dice_sums.cpu().numpy().astype(np.float64)
        assert abs(float(dice_from_sums(s[0], s[1], s[2], 1.0)) - D) <= 2e-5
    assert bool(torch.any(m.net.flat_w != w0)) and bool(torch.all(torch.isfinite(m.net.flat_w)))
    assert Ds[-1] > Ds[0], (Ds[0], Ds[-1])
