"""-m gpu: the weighted cross-entropy head (rsu.h rsu_head_fwd_bwd_w: class weights, a per-pixel weight map, ignored labels) through the
C ABI against the CPU checker's unweighted functions plus the three lines that define the weights, its bit-equality with
rsu_head_fwd_bwd when every weight is 1, and the network / model level above it. Tolerances are tests/test_gpu_ops.py::test_head's."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import unet_oracle as U  # noqa: E402
from tests import hiputil as hu  # noqa: E402
from tests.head_util import NETS, NPIX, RSU_EINVAL, _batch, _bits, _inputs, _model, _net, _weight_map  # noqa: E402
from tests.head_util import _step as head_step  # noqa: E402
from road_segmentation_unet_amd._lib import RsuError, call, lib  # noqa: E402



class Out:
    def __init__(self, C, fill=0.0):
        z = lambda *s, dtype=torch.float32: torch.full(s, fill, dtype=dtype, device=hu.DEV)  # noqa: E731
        self.prob, self.dact = z(NPIX), z(NPIX, C, dtype=torch.bfloat16)
        self.dw, self.db = z(C, 2), z(2)
        self.loss, self.wsum = torch.zeros(1, device=hu.DEV), torch.zeros(1, device=hu.DEV)

    def all(self):
        return [("prob", self.prob), ("dact", self.dact), ("dw", self.dw), ("db", self.db), ("loss_sum", self.loss), ("weight_sum", self.wsum)]


def _run_w(C, act_d, w_d, b_d, labels, class_w, pixel_w, inv, want_wsum=True):
    o = Out(C)
    ws = torch.zeros(lib().rsu_head_w_ws_floats(NPIX, C), dtype=torch.float32, device=hu.DEV)
    lab = torch.from_numpy(np.ascontiguousarray(labels, dtype=np.int64)).to(hu.DEV)
    cw = hu.dev_f32(np.asarray(class_w, np.float32)) if class_w is not None else None
    pw = hu.dev_f32(pixel_w) if pixel_w is not None else None
    call("rsu_head_fwd_bwd_w", hu.ptr(act_d), hu.ptr(w_d), hu.ptr(b_d), hu.ptr(lab), hu.ptr(cw), hu.ptr(pw), hu.ptr(o.prob), hu.ptr(o.loss),
         hu.ptr(o.wsum) if want_wsum else None, hu.ptr(o.dact), hu.ptr(o.dw), hu.ptr(o.db), hu.ptr(ws), NPIX, C, inv, hu.stream())
    torch.cuda.synchronize()
    return o


def _check_against_reference(o, act, w, b, labels, omega, what):
    """the reference: the checker's unweighted head (as test_head uses it) + rdl * omega, sum(omega * ce), omega.sum()"""
    valid = (labels == 0) | (labels == 1)
    assert np.all(omega[~valid] == 0)
    ref_labels = np.where(valid, labels, 0)     # (an ignored pixel has omega = 0: the label the checker sees there is immaterial)
    ref_logits = U.conv1x1_fwd(act, w, b)
    rp, _, rdl = U.softmax_ce(ref_logits, ref_labels)
    z = ref_logits.astype(np.float64)
    zmax = z.max(axis=1)
    ce = zmax + np.log(np.exp(z - zmax[:, None]).sum(axis=1)) - z[np.arange(NPIX), ref_labels]
    rdl_w = (rdl * 0.5) * omega[:, None].astype(np.float32)   # the checker's dlogits are / npix; the call scales by 1 / (2 npix)
    loss_w = float(np.sum(omega.astype(np.float64) * ce))
    wsum = float(omega.astype(np.float64).sum())
    rdx, rdw, rdb = U.conv1x1_bwd(act, w, rdl_w)
    got_loss, got_wsum = float(hu.host(o.loss)[0]), float(hu.host(o.wsum)[0])
    print("%s: loss/npix got %.9g ref %.9g; weight_sum got %.9g ref %.9g" % (what, got_loss / NPIX, loss_w / NPIX, got_wsum, wsum))
    hu.assert_f32_close(hu.host(o.prob), rp, what + " prob", rtol=1e-4, atol_scale=1e-6)
    assert abs(got_loss / NPIX - loss_w / NPIX) < 2e-5 * max(1.0, abs(loss_w / NPIX)), (what, got_loss, loss_w)
    assert abs(got_wsum - wsum) <= 2e-5 * abs(wsum), (what, got_wsum, wsum)
    hu.assert_bf16_close(hu.host(o.dact), U.relu_bwd(act, rdx), what + " dact")
    hu.assert_f32_close(hu.host(o.dw), rdw, what + " dw")
    hu.assert_f32_close(hu.host(o.db), rdb, what + " db")


# ------------------------------------------------------------------------------------------- the op
@pytest.mark.parametrize("C", [64, 16])
@pytest.mark.parametrize("mode", ["class", "map", "both"])
def test_weighted_head_against_reference(C, mode):
    rng, act, w, b, labels = _inputs(C)
    class_w = (0.6, 2.5) if mode in ("class", "both") else None
    pixel_w = _weight_map(rng) if mode in ("map", "both") else None
    omega = np.ones(NPIX, np.float32)
    if class_w is not None:
        omega = omega * np.asarray(class_w, np.float32)[labels]
    if pixel_w is not None:
        assert (pixel_w == 0).sum() > 0
        omega = omega * pixel_w
    o = _run_w(C, hu.dev_bf16(act), hu.dev_f32(w), hu.dev_f32(b), labels, class_w, pixel_w, 1.0 / (2 * NPIX))
    _check_against_reference(o, act, w, b, labels, omega, "weighted head (%s, C=%d)" % (mode, C))


@pytest.mark.parametrize("C", [64, 16])
def test_ignored_labels(C):
    rng, act, w, b, labels = _inputs(C)
    class_w, pixel_w = (0.6, 2.5), _weight_map(rng)
    labels = labels.copy()
    ign = rng.rand(NPIX) < 0.10
    labels[ign] = -1
    few = rng.choice(np.nonzero(~ign)[0], 6, replace=False)
    labels[few[:5]] = 255
    labels[few[5]] = 2 ** 32 + 1          # its low 32 bits are a valid label
    ign = (labels != 0) & (labels != 1)
    assert ign.sum() > NPIX // 20
    omega = np.where(ign, 0.0, np.asarray(class_w, np.float32)[np.where(ign, 0, labels)] * pixel_w).astype(np.float32)
    ad, wd, bd = hu.dev_bf16(act), hu.dev_f32(w), hu.dev_f32(b)
    inv = 1.0 / (2 * NPIX)
    o = _run_w(C, ad, wd, bd, labels, class_w, pixel_w, inv)
    _check_against_reference(o, act, w, b, labels, omega, "ignored labels (C=%d)" % C)
    rows = o.dact[torch.from_numpy(ign).to(hu.DEV)]
    assert rows.shape[0] == int(ign.sum()) and not torch.any(rows != 0), "dact rows of ignored pixels must be exactly 0"
    # what an ignored pixel carries besides "ignored" must not reach any output: another weight and another ignored label there
    labels2, pixel_w2 = labels.copy(), pixel_w.copy()
    labels2[ign] = np.where(labels[ign] == -1, 7, -(2 ** 40))
    pixel_w2[ign] = (3.0 + 100.0 * rng.rand(int(ign.sum()))).astype(np.float32)
    pixel_w2[np.nonzero(ign)[0][:3]] = [np.inf, np.nan, -1e30]
    o2 = _run_w(C, ad, wd, bd, labels2, class_w, pixel_w2, inv)
    for (name, t), (_, t2) in zip(o.all(), o2.all()):
        assert torch.equal(_bits(t), _bits(t2)), name


@pytest.mark.parametrize("C", [64, 16])
def test_all_ones_equals_unweighted_head_bit_for_bit(C):
    _, act, w, b, labels = _inputs(C)
    ad, wd, bd = hu.dev_bf16(act), hu.dev_f32(w), hu.dev_f32(b)
    inv = 1.0 / (2 * NPIX)
    ref = Out(C)
    ws = torch.zeros(lib().rsu_head_ws_floats(NPIX, C), dtype=torch.float32, device=hu.DEV)
    lab = torch.from_numpy(labels).to(hu.DEV)
    call("rsu_head_fwd_bwd", hu.ptr(ad), hu.ptr(wd), hu.ptr(bd), hu.ptr(lab), hu.ptr(ref.prob), hu.ptr(ref.loss), hu.ptr(ref.dact), hu.ptr(ref.dw),
         hu.ptr(ref.db), hu.ptr(ws), NPIX, C, inv, hu.stream())
    torch.cuda.synchronize()
    assert float(ref.loss.item()) > 0
    for class_w, pixel_w in (((1.0, 1.0), np.ones(NPIX, np.float32)), (None, None)):
        o = _run_w(C, ad, wd, bd, labels, class_w, pixel_w, inv)
        for (name, t), (_, r) in zip(o.all()[:5], ref.all()[:5]):
            assert torch.equal(_bits(t), _bits(r)), (name, class_w)
        assert float(o.wsum.item()) == float(NPIX)      # (a sum of ones: exact below 2^24)
    # weight_sum is optional
    o = _run_w(C, ad, wd, bd, labels, None, None, inv, want_wsum=False)
    assert torch.equal(_bits(o.loss), _bits(ref.loss)) and float(o.wsum.item()) == 0.0


def test_weighted_head_argument_checks():
    C = 16
    _, act, w, b, labels = _inputs(C)
    ad, wd, bd = hu.dev_bf16(act), hu.dev_f32(w), hu.dev_f32(b)
    lab = torch.from_numpy(labels).to(hu.DEV)
    o = Out(C, fill=7.0)
    o.loss.fill_(7.0)
    o.wsum.fill_(7.0)
    ws = torch.full((lib().rsu_head_w_ws_floats(NPIX, C),), 7.0, dtype=torch.float32, device=hu.DEV)
    assert lib().rsu_head_w_ws_floats(NPIX, C) > lib().rsu_head_ws_floats(NPIX, C)

    def rc(act=ad, labels=lab, ws=ws, C=C, npix=NPIX):
        return lib().rsu_head_fwd_bwd_w(hu.ptr(act), hu.ptr(wd), hu.ptr(bd), hu.ptr(labels), None, None, hu.ptr(o.prob), hu.ptr(o.loss),
                                        hu.ptr(o.wsum), hu.ptr(o.dact), hu.ptr(o.dw), hu.ptr(o.db), hu.ptr(ws), npix, C, 0.5 / NPIX, hu.stream())
    assert rc(act=None) == RSU_EINVAL
    assert rc(labels=None) == RSU_EINVAL
    assert rc(ws=None) == RSU_EINVAL
    for bad_c in (0, 12, 24, 520):
        assert rc(C=bad_c) == RSU_EINVAL, bad_c
    assert rc(npix=0) == RSU_EINVAL
    assert rc(npix=-5) == RSU_EINVAL
    torch.cuda.synchronize()
    for name, t in o.all() + [("ws", ws)]:
        assert bool(torch.all(t == 7.0)), "%s was written by a refused call" % name


# ------------------------------------------------------------------------------------------- the network
def _step(m):
    return head_step(m)[:4]   # (without the Dice sums)


@pytest.mark.parametrize("L,root,dilated,P", NETS)
def test_net_default_call_for_none_and_unit_class_weights(L, root, dilated, P):
    a, b = _net(L, root, dilated, P, None), _net(L, root, dilated, P, (1.0, 1.0))
    assert not a.loss_is_weighted() and not b.loss_is_weighted()
    _batch(a)
    _batch(b)
    ga, pa, la, _ = _step(a)
    gb, pb, lb, _ = _step(b)
    assert torch.equal(_bits(ga), _bits(gb)) and torch.equal(_bits(pa), _bits(pb)) and torch.equal(_bits(la), _bits(lb))
    assert float(la.item()) > 0 and bool(torch.any(ga != 0))


@pytest.mark.parametrize("L,root,dilated,P", NETS)
def test_net_class_weights_two_two_doubles_every_gradient_exactly(L, root, dilated, P):
    """a power-of-two factor commutes with every rounding downstream of the head (bf16 stores, MFMA fp32 accumulation, split sums)"""
    a, b = _net(L, root, dilated, P, None), _net(L, root, dilated, P, (2.0, 2.0))
    assert b.loss_is_weighted()
    _batch(a)
    _batch(b)
    ga, pa, la, _ = _step(a)
    gb, pb, lb, wb = _step(b)
    n = a.n_live
    nz = ga[:n][ga[:n] != 0].abs()
    print("smallest non-zero |gradient| %.3g, largest %.3g" % (float(nz.min()), float(nz.max())))
    assert torch.equal(_bits(gb[:n]), _bits(2.0 * ga[:n]))
    assert torch.equal(_bits(lb), _bits(2.0 * la))
    assert torch.equal(_bits(pa), _bits(pb))
    assert float(wb.item()) == 2.0 * a.B * P * P


@pytest.mark.parametrize("L,root,dilated,P", NETS)
def test_net_zero_weight_patch_equals_ignored_patch(L, root, dilated, P):
    """two routes to the same omega: a weight map that is 0 on patch 1, or the labels of patch 1 set to -1 (compared as numbers: 0 * x
    may be -0 where the ignore path stores +0)"""
    cw = (0.6, 2.5)
    a, b = _net(L, root, dilated, P, cw), _net(L, root, dilated, P, cw)
    _batch(a)
    _batch(b)
    wmap = torch.ones((2, P, P))
    wmap[1] = 0.0
    a.set_pixel_weights(wmap)
    b.labels[1] = -1
    assert a.loss_is_weighted() and b.loss_is_weighted() and b.pixel_weights is None
    ga, _, la, wa = _step(a)
    gb, _, lb, wb = _step(b)
    assert torch.equal(ga, gb) and torch.equal(la, lb) and torch.equal(wa, wb)
    assert float(wa.item()) > 0 and bool(torch.any(ga != 0))


@pytest.mark.parametrize("L,root,dilated,P", NETS)
def test_net_weighted_step_is_deterministic_and_tune_keeps_the_map(L, root, dilated, P):
    m = _net(L, root, dilated, P, (0.6, 2.5))
    _batch(m)
    gen = torch.Generator(device="cpu").manual_seed(3)
    wmap = 0.25 + torch.rand((2, P, P), generator=gen)
    m.set_pixel_weights(wmap)
    m.labels[0, :3] = -1
    m.tune()
    assert m.pixel_weights is not None and torch.equal(m.pixel_weights.cpu(), wmap)
    assert int((m.labels == -1).sum()) == 3 * P
    first = _step(m)
    second = _step(m)
    for x, y in zip(first, second):
        assert torch.equal(_bits(x), _bits(y))
    m.set_pixel_weights(None)
    assert m.pixel_weights is None and m.loss_is_weighted()
    m.class_weights = None
    assert not m.loss_is_weighted()
    with pytest.raises(RsuError):
        m.class_weights = (0.0, 0.0)
    with pytest.raises(RsuError):
        m.set_pixel_weights(torch.ones((2, P + 1, P)))


# ------------------------------------------------------------------------------------------- the model
def test_model_train_step_with_class_weights_and_a_map():
    m = _model(class_weights="1,3")
    assert m.net.class_weights == (1.0, 3.0)
    rng = np.random.RandomState(2)
    S = m.input_size
    w0 = m.net.flat_w.clone()
    for step in range(3):
        X = rng.rand(2, S, S, 3).astype(np.float32)
        y = (rng.rand(2, 20, 20) < 0.3).astype(np.int64)
        wmap = (0.25 + rng.rand(2, 20, 20)).astype(np.float32) if step != 1 else None
        loss, prob = m.train_step(X, y, weights=wmap)
        assert (m.net.pixel_weights is None) == (wmap is None)
        assert np.isfinite(float(loss)) and float(loss) > 0
        assert float(m.net.weight_sum.item()) > 0
    assert bool(torch.any(m.net.flat_w != w0)) and bool(torch.all(torch.isfinite(m.net.flat_w)))


def test_model_refuses_unresolved_balanced_weights():
    with pytest.raises(ValueError):
        _model(class_weights="balanced")
