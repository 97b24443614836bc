"""-m gpu: the clDice term (include/rsu_cldice.h) through the C ABI. Three levels, held separately (the device's prob differs from a float64
prob in the last bit, which can re-route a gradient at a near-tie, so the composed op is never compared with autograd from the
activations): (1) rsu_cldice_fwd's skeletons against hostio.soft_skeleton bit for bit and its sums against hostio.cldice_gradient;
(2) rsu_cldice_bwd's gprob against hostio.cldice_gradient -- float64, the tie rule of the header, computed from the identical float32
prob -- on tie-free, tied and saturated maps with ignored labels; (3) rsu_head_fwd_bwd_aux against float64 autograd with the linear term
sum gprob_i p_i, gprob given. Then determinism, accumulation, argument errors, and the network / model level above them.
Tolerances: hiputil.assert_f32_close's defaults for gprob, 2e-5 relative for scalar sums, tests/test_gpu_focal.py's for the head."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import cldice_util as CU  # noqa: E402
from tests import hiputil as hu  # noqa: E402
from tests.head_util import LAM, NETS, NPIX, RSU_EINVAL, SMOOTH, _batch, _bits, _model, _net, _step  # noqa: E402
from tests.test_gpu_focal import INV, MODES, Dev, Out, _case, _check, _train  # noqa: E402
from road_segmentation_unet_amd import hostio  # noqa: E402
from road_segmentation_unet_amd._lib import RsuError, call, lib  # noqa: E402

KINDS = ["tie_free", "tied4", "tied8", "tied16", "saturated"]


@functools.lru_cache(maxsize=None)
def _maps(shape, kind):
    if kind.startswith("tied"):
        return CU.tied(shape, int(kind[4:]))
    return CU.tie_free(shape) if kind == "tie_free" else CU.saturated(shape)


@functools.lru_cache(maxsize=None)
def _ref(shape, kind, iters):
    """(skeletons float32, (skel_p, skel_y, sums, gprob) float64): computed once per case and never written"""
    p, labels = _maps(shape, kind)
    y = (labels == 1).astype(np.float32)
    return hostio.soft_skeleton(p, iters), hostio.soft_skeleton(y, iters), hostio.cldice_gradient(p, labels, iters, CU.SCALE, CU.SMOOTH)


def _bufs(shape, iters, p, labels, fill=0.0):
    n = int(np.prod(shape))
    z = lambda *s: torch.full(s, fill, dtype=torch.float32, device=hu.DEV)  # noqa: E731
    return {"prob": hu.dev_f32(p), "labels": torch.from_numpy(labels).to(hu.DEV), "skel_p": z(*shape), "skel_y": z(*shape), "gprob": z(*shape),
            "sums": torch.zeros(4, dtype=torch.float32, device=hu.DEV), "ws": z(CU.ws_floats(shape, iters)), "n": n}


def _run(shape, iters, p, labels):
    b = _bufs(shape, iters, p, labels, fill=float("nan"))
    CU.run_fwd(b, iters, shape, hu.stream())
    CU.run_bwd(b, iters, CU.SCALE, CU.SMOOTH, shape, hu.stream())
    torch.cuda.synchronize()
    return b


# ------------------------------------------------------------------------------------------- 1. + 2. skeletons, sums, gradient
@pytest.mark.parametrize("shape,iters", CU.CASES, ids=["%dx%dx%d-k%d" % (s + (k,)) for s, k in CU.CASES])
def test_skeletons_sums_and_gradient(shape, iters):
    assert lib().rsu_cldice_ws_floats(*shape, iters) > 0
    for kind in KINDS:
        p, labels = _maps(shape, kind)
        sp32, sy32, (sp, sy, sums, gprob) = _ref(shape, kind, iters)
        b = _run(shape, iters, p, labels)
        what = "clDice %s %s k=%d" % (shape, kind, iters)
        got_p, got_y = b["skel_p"].cpu().numpy(), b["skel_y"].cpu().numpy()
        assert np.array_equal(got_p.view(np.int32), sp32.view(np.int32)), what + ": skel_p bits"
        assert np.array_equal(got_y.view(np.int32), sy32.view(np.int32)), what + ": skel_y bits"
        got_sums = b["sums"].cpu().numpy().astype(np.float64)
        g = b["gprob"].cpu().numpy()
        print("%s: sums got %s ref %s; max|g| %.3g skel>0 %.2f g!=0 %.2f" % (what, got_sums, sums, np.abs(gprob).max(), (sp > 0).mean(),
                                                                             (gprob != 0).mean()))
        assert np.all(np.abs(got_sums - sums) <= 2e-5 * np.abs(sums)), (what, got_sums, sums)
        hu.assert_f32_close(g, gprob, what + " gprob")
        ign = (labels != 0) & (labels != 1)
        assert not g[ign].any() and not np.signbit(g[ign]).any(), what + ": ignored pixels are constants"
        # the reference is not trivial. (iters = 0 is left out: a one-level skeleton of the REFERENCE reaches fewer pixels whatever the
        # kernel does -- skel > 0 at 36 %, gprob != 0 at 44 % of (3, 37, 41), 10 % of them ignored; from iters = 1 on it is 41 / 56 % and more)
        if kind == "tie_free" and shape in ((3, 37, 41), (2, 70, 67)) and iters >= 1:
            assert (sp > 0).mean() >= 0.20 and (gprob != 0).mean() >= 0.50, (what, (sp > 0).mean(), (gprob != 0).mean())


def test_the_tie_rule_is_seen():
    """on a tied map torch's own sub-gradient (a tie of the cross split in halves) is far outside what the kernel is granted"""
    shape, iters = (3, 37, 41), 3
    p, labels = _maps(shape, "tied4")
    g = _run(shape, iters, p, labels)["gprob"].cpu().numpy()
    tg = CU.torch_cldice(p, labels, iters, CU.SCALE, CU.SMOOTH)[3]
    assert (np.abs(g - tg) > 1e-4 * np.abs(tg) + 1e-5 * np.abs(tg).max()).mean() > 0.10


# ------------------------------------------------------------------------------------------- determinism, accumulation, given sums
@pytest.mark.parametrize("iters", [3, 16])
def test_determinism_accumulation_and_given_sums(iters):
    shape = (3, 37, 41)
    p, labels = _maps(shape, "saturated")
    a, b = _run(shape, iters, p, labels), _run(shape, iters, p, labels)
    for n in ("skel_p", "skel_y", "sums", "gprob", "ws"):
        assert torch.equal(_bits(a[n]), _bits(b[n])), n
    once = a["sums"].clone()
    CU.run_fwd(a, iters, shape, hu.stream())     # on top of the first: += doubles (x + x is exact)
    torch.cuda.synchronize()
    assert torch.equal(a["sums"], 2 * once) and float(once.min()) > 0
    # the backward follows the sums it is given: it recomputes none of them
    given = np.array([3.0, 11.0, 5.0, 7.0])
    b["given"] = hu.dev_f32(given)
    CU.run_bwd(b, iters, CU.SCALE, CU.SMOOTH, shape, hu.stream(), sums="given")
    ref = hostio.cldice_gradient(p, labels, iters, CU.SCALE, CU.SMOOTH, sums=given)[3]
    hu.assert_f32_close(b["gprob"].cpu().numpy(), ref, "gprob from given sums k=%d" % iters)
    assert np.abs(ref - _ref(shape, "saturated", iters)[2][3]).max() > 1e-2 * np.abs(ref).max()


# ------------------------------------------------------------------------------------------- argument errors
def test_argument_errors_leave_every_output_untouched():
    shape, iters = (2, 9, 11), 3
    p, labels = CU.tie_free(shape)
    b = _bufs(shape, iters, p, labels, fill=7.0)
    b["sums"].fill_(7.0)
    L, P, st = lib(), hu.ptr, hu.stream()
    outs = ("skel_p", "skel_y", "sums", "gprob", "ws")
    before = {n: b[n].clone() for n in outs}
    fwd = [P(b["prob"]), P(b["labels"]), iters, P(b["skel_p"]), P(b["skel_y"]), P(b["sums"]), P(b["ws"]), 2, 9, 11, st]
    bwd = [P(b["prob"]), P(b["labels"]), P(b["skel_p"]), P(b["skel_y"]), P(b["sums"]), iters, 0.5, 1.0, P(b["gprob"]), P(b["ws"]), 2, 9, 11, st]

    def bad(args, i, v):
        a = list(args)
        a[i] = v
        return a
    cases = [("rsu_cldice_fwd", bad(fwd, i, None)) for i in (0, 1, 3, 4, 5, 6)]
    cases += [("rsu_cldice_fwd", bad(fwd, i, v)) for i, v in ((2, -1), (2, 17), (7, 0), (8, 0), (9, 0), (7, -1), (7, 1 << 30))]
    cases += [("rsu_cldice_bwd", bad(bwd, i, None)) for i in (0, 1, 2, 3, 4, 8, 9)]
    cases += [("rsu_cldice_bwd", bad(bwd, i, v)) for i, v in ((5, -1), (5, 17), (10, 0), (11, 0), (12, -3), (10, 1 << 30))]
    cases += [("rsu_cldice_bwd", bad(bwd, 6, v)) for v in (-1e-3, float("nan"), float("inf"))]
    cases += [("rsu_cldice_bwd", bad(bwd, 7, v)) for v in (0.0, -1.0, float("nan"), float("inf"))]
    for name, args in cases:
        assert getattr(L, name)(*args) == RSU_EINVAL, (name, args)
    assert L.rsu_cldice_ws_floats(2, 9, 11, 17) == 0 and L.rsu_cldice_ws_floats(0, 9, 11, 3) == 0 and L.rsu_cldice_ws_floats(1 << 30, 9, 11, 3) == 0
    # the aux head: whatever the focal entry refuses, except gamma == 0, and a NULL gprob
    act, w, bb, lab, class_w, pixel_w, _ = _case(16, "ignored")
    d, o = Dev(16, act, w, bb, lab, class_w, pixel_w), Out(16, fill=7.0, acc=7.0)
    gp = torch.zeros(NPIX, dtype=torch.float32, device=hu.DEV)
    aux = [*d.head(), P(d.cw), P(d.pw), 2.0, P(o.sums), LAM, SMOOTH, P(o.prob), P(o.loss), P(o.wsum), P(o.dact), P(o.dw), P(o.db), P(d.ws_t),
           NPIX, 16, INV, P(gp), st]
    keep = [(n, t.clone()) for n, t in o.all()]
    for i, v in [(i, None) for i in (0, 1, 2, 3, 10, 11, 13, 14, 15, 16, 20)] + [(6, -1.0), (6, float("nan")), (6, float("inf")), (17, 0), (18, 12),
                                                                                 (18, 1024), (8, -1.0), (8, float("nan")), (9, 0.0), (9, float("inf"))]:
        assert L.rsu_head_fwd_bwd_aux(*bad(aux, i, v)) == RSU_EINVAL, (i, v)
    torch.cuda.synchronize()
    for n in outs:
        assert torch.equal(_bits(b[n]), _bits(before[n])), n
    for (n, t), (_, k) in zip(o.all(), keep):
        assert torch.equal(t, k), n
    assert L.rsu_head_fwd_bwd_aux(*bad(aux, 6, 0.0)) == 0          # gamma == 0 is allowed
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- 3. the aux head
def _gprob(C, ign, poison=False):
    rng = np.random.RandomState(100 + C)
    g = (rng.standard_normal(NPIX) * 4.0 * INV).astype(np.float32)
    if poison:   # an ignored pixel's gprob is never looked at
        idx = np.nonzero(ign)[0]
        g[idx[0::3]], g[idx[1::3]], g[idx[2::3]] = np.inf, np.nan, -np.inf
    return g


def _aux(d, gamma, dice, gprob, o=None):
    o = o or Out(d.C)
    p = hu.ptr
    if dice:
        call("rsu_head_dice_sums", *d.head(), p(d.pw), p(o.prob_a), p(o.sums), p(d.ws_t), NPIX, d.C, hu.stream())
    call("rsu_head_fwd_bwd_aux", *d.head(), p(d.cw), p(d.pw), gamma, p(o.sums) if dice else None, LAM, SMOOTH, p(o.prob), p(o.loss), p(o.wsum),
         p(o.dact), p(o.dw), p(o.db), p(d.ws_t), NPIX, d.C, INV, p(gprob), hu.stream())
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("dice", [False, True], ids=["plain", "dice"])
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("gamma", [0.0, 2.0])
@pytest.mark.parametrize("C", [64, 16])
def test_aux_head_against_float64_autograd(C, gamma, mode, dice):
    act, w, b, labels, class_w, pixel_w, ign = _case(C, mode)
    d = Dev(C, act, w, b, labels, class_w, pixel_w)
    gp = _gprob(C, ign, poison=True)
    o = _aux(d, gamma, dice, hu.dev_f32(gp))
    safe_pw = None if pixel_w is None else np.where(ign, 1.0, pixel_w)
    ref = CU.AuxRef(act, w, b, labels, class_w, safe_pw, INV, gamma, gp, lam=LAM if dice else 0.0, smooth=SMOOTH)
    ref.ce_sum = ref.loss_sum
    what = "aux head (C=%d, gamma=%g, %s%s)" % (C, gamma, mode, ", dice" if dice else "")
    _check(o, ref, what, ign)       # (ignored rows of dact exactly +0 whatever gprob holds there: inf and NaN included)
    without = CU.AuxRef(act, w, b, labels, class_w, safe_pw, INV, gamma, np.zeros(NPIX), lam=LAM if dice else 0.0, smooth=SMOOTH)
    assert float(np.abs(ref.dw - without.dw).max()) > 1e-2 * float(np.abs(without.dw).max())
    assert ref.loss_sum == without.loss_sum          # loss_sum keeps its meaning: the cross-entropy part


@pytest.mark.parametrize("C", [64, 16])
def test_aux_head_with_a_zero_gprob_is_the_sibling(C):
    act, w, b, labels, class_w, pixel_w, _ = _case(C, "ignored")
    d = Dev(C, act, w, b, labels, class_w, pixel_w)
    zero = torch.zeros(NPIX, dtype=torch.float32, device=hu.DEV)
    for gamma, dice, sibling in ((0.0, False, "rsu_head_fwd_bwd_w"), (0.0, True, "rsu_head_fwd_bwd_dice"), (2.0, False, "rsu_head_fwd_bwd_focal"),
                                 (2.0, True, "rsu_head_fwd_bwd_focal")):
        got, ref = _aux(d, gamma, dice, zero), _train(d, gamma, dice, entry=sibling)
        assert float(ref.loss.item()) > 0
        for (name, t), (_, r) in zip(got.all()[:8], ref.all()[:8]):
            assert torch.equal(t.to(torch.float32), r.to(torch.float32)), (sibling, name)      # as numbers: only a zero's sign may differ


# ------------------------------------------------------------------------------------------- the network level
@pytest.mark.parametrize("L,root,dilated,P", NETS)
def test_net_without_the_term_is_the_default_net(L, root, dilated, P):
    a, b = _net(L, root, dilated, P), _net(L, root, dilated, P, cldice_weight=0.0, cldice_iters=3, cldice_smooth=2.0)
    assert b.cldice_sums is None and b.gprob is None and b._cldice_ws is None        # no buffer without the term
    outs = []
    for m in (a, b):
        _batch(m)
        outs.append(_step(m))
    for x, y in zip(*outs):
        assert torch.equal(_bits(x), _bits(y))


@pytest.mark.parametrize("focal,dice", [(0.0, 0.0), (2.0, 0.0), (0.0, LAM), (2.0, LAM)], ids=["ce", "focal", "dice", "focal+dice"])
@pytest.mark.parametrize("L,root,dilated,P", NETS)
def test_net_runs_the_stand_alone_sequence(L, root, dilated, P, focal, dice):
    """the net's prob, skeletons, cldice_sums, gprob and head gradients against the entries called one by one on the same buffers"""
    lam, iters = 0.8, 3
    m = _net(L, root, dilated, P, class_weights=(0.6, 2.5), dice_weight=dice, focal_gamma=focal, cldice_weight=lam, cldice_iters=iters)
    _batch(m)
    m.labels.view(-1)[::7] = -1
    inv = 1.0 / (m.B * P * P)
    _step(m)
    assert float(m.cldice_sums.min()) > 0 and bool(torch.any(m.gprob != 0))
    shape, npix, C, st = (m.B, P, P), m.B * P * P, root, hu.stream()
    p = hu.ptr
    z = lambda *s, dtype=torch.float32: torch.full(s, float("nan"), dtype=dtype, device=hu.DEV)  # noqa: E731
    o = {"prob": z(*shape), "labels": m.labels, "skel_p": z(*shape), "skel_y": z(*shape), "gprob": z(*shape),
         "sums": torch.zeros(4, dtype=torch.float32, device=hu.DEV), "ws": z(CU.ws_floats(shape, iters))}
    dsums, loss, wsum = z(3), torch.zeros(1, device=hu.DEV), torch.zeros(1, device=hu.DEV)
    dact, dw, db = z(npix, C, dtype=torch.bfloat16), z(C, 2), z(2)
    ws = torch.zeros(lib().rsu_head_dice_ws_floats(npix, C), dtype=torch.float32, device=hu.DEV)
    head = (p(m.act[m.last_name]), p(m.w["weight_output/kernel"]), p(m.w["weight_output/bias"]))
    if dice:
        call("rsu_head_dice_sums", *head, p(m.labels), None, p(o["prob"]), p(dsums), p(ws), npix, C, st)
    else:
        call("rsu_head_fwd", *head, p(o["prob"]), None, npix, C, st)
    CU.run_fwd(o, iters, shape, st)
    CU.run_bwd(o, iters, lam, 1.0, shape, st)
    call("rsu_head_fwd_bwd_aux", *head, p(m.labels), p(m._class_w_dev), None, focal, p(dsums) if dice else None, dice, SMOOTH, p(o["prob"]), p(loss),
         p(wsum), p(dact), p(dw), p(db), p(ws), npix, C, inv, p(o["gprob"]), st)
    torch.cuda.synchronize()
    pairs = [("prob", m.prob, o["prob"]), ("skel_p", m.skel_p, o["skel_p"]), ("skel_y", m.skel_y, o["skel_y"]), ("sums", m.cldice_sums, o["sums"]),
             ("gprob", m.gprob, o["gprob"]), ("dact", m.grad[m.last_name].reshape(npix, C), dact), ("dw", m.g["weight_output/kernel"].reshape(C, 2), dw),
             ("db", m.g["weight_output/bias"], db), ("loss_sum", m.loss_sum, loss), ("weight_sum", m.weight_sum, wsum)]
    for name, got, ref in pairs:
        assert torch.equal(_bits(got), _bits(ref)), name
    # and the term reaches the whole net's gradient
    g1 = m.flat_g.clone()
    _step(m, cldice_scale=0.0)
    assert float((g1 - m.flat_g).abs().max()) > 1e-3 * float(m.flat_g.abs().max())
    # the evaluation pass adds the same four sums to its own accumulator
    m.reset_eval()
    m.forward_device(keep=1.0)
    m.evaluate_device()
    m.evaluate_device()
    torch.cuda.synchronize()
    assert torch.equal(m.eval_cldice_sums, 2 * o["sums"])
    m.reset_eval()
    assert not bool(m.eval_cldice_sums.any())


def test_net_refuses_bad_values():
    L, root, dilated, P = NETS[1]
    for kw in ({"cldice_weight": -1.0}, {"cldice_weight": float("nan")}, {"cldice_weight": "x"}, {"cldice_iters": 17}, {"cldice_iters": -1},
               {"cldice_iters": 2.5}, {"cldice_iters": True}, {"cldice_smooth": 0.0}, {"cldice_smooth": float("inf")}):
        with pytest.raises(RsuError):
            _net(L, root, dilated, P, **kw)
    from road_segmentation_unet_amd.unet import UNet
    with pytest.raises(RsuError):
        UNet(L, root, dilated, 2, P, seed=17, training=False, cldice_weight=1.0)
    m = _net(L, root, dilated, P, cldice_weight=0.5)
    _batch(m)
    m.forward_device()
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(RsuError):
            m.backward_device(1.0 / (m.B * P * P), cldice_scale=bad)
    for name, bad in (("cldice_weight", -1), ("cldice_iters", 99), ("cldice_smooth", 0)):
        with pytest.raises(RsuError):
            setattr(m, name, bad)
    assert (m.cldice_weight, m.cldice_iters, m.cldice_smooth) == (0.5, 10, 1.0)


# ------------------------------------------------------------------------------------------- the model level
def _stripes(m):
    """the batch of tests/test_gpu_dice_loss.py::test_model_trains_with_the_dice_term"""
    rng = np.random.RandomState(2)
    S, P = m.input_size, 20
    ii, jj = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    stripes = (((ii + jj) // 5) % 2).astype(np.float32)
    X = rng.rand(2, S, S, 3).astype(np.float32)
    X[1] = X[1, ::-1]
    masks = np.stack([stripes, stripes[::-1]])
    X[..., 0] = 0.1 + 0.8 * masks + 0.1 * X[..., 0]
    off = (S - P) // 2
    return X, masks[:, off:off + P, off:off + P].astype(np.int64)


def test_model_trains_with_the_cldice_term():
    """thirty steps on the stripes batch at lambda = 1: the logged loss is cross-entropy + (1 - clD) with clD from the device sums, the
    objective falls and clD rises"""
    from road_segmentation_unet_amd.model import cldice_from_sums
    m = _model(cldice_weight=1.0, cldice_iters=3)
    assert (m.net.cldice_weight, m.net.cldice_iters, m.net.cldice_smooth) == (1.0, 3, 1.0)
    X, y = _stripes(m)
    w0 = m.net.flat_w.clone()
    losses, cls = [], []
    for step in range(30):
        loss, prob = m.train_step(X, y)
        pr = prob.cpu().numpy()
        _, _, sums, _ = hostio.cldice_gradient(pr, y, 3, 1.0, 1.0)
        cl = float(cldice_from_sums(*sums, 1.0))
        p1 = pr.astype(np.float64)
        ce = float(-np.log(np.where(y == 1, p1, 1.0 - p1)).mean())
        got = float(loss)
        print("step %2d: loss %.7f host %.7f  clD %.5f" % (step, got, ce + 1.0 - cl, cl))
        assert abs(got - (ce + 1.0 - cl)) <= 1e-5 * max(1.0, abs(got)), (step, got, ce, cl)
        s = m.net.cldice_sums.cpu().numpy().astype(np.float64)
        assert abs(float(cldice_from_sums(*s, 1.0)) - cl) <= 2e-5
        losses.append(got)
        cls.append(cl)
    assert bool(torch.any(m.net.flat_w != w0)) and bool(torch.all(torch.isfinite(m.net.flat_w)))
    assert losses[-1] < losses[0] and cls[-1] > cls[0], (losses[0], losses[-1], cls[0], cls[-1])


def test_evaluate_reports_cldice():
    from road_segmentation_unet_amd.model import cldice_from_sums
    plain, m = _model(), _model(cldice_weight=0.5, cldice_iters=3)
    X, y = _stripes(m)
    X, y = np.concatenate([X, X[::-1]]), np.concatenate([y, y[::-1]])[:3]
    X = X[:3]                                   # three patches at a batch of two: the last chunk is padded with ignored labels
    a, b = plain.evaluate(X, y), m.evaluate(X, y)
    assert a["cldice"] == 1.0 and not a["cldice_sums"].any() and a["cldice_sums"].shape == (4,)
    for k in a:
        if k not in ("objective", "cldice", "cldice_sums"):
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    assert b["cldice_sums"].shape == (4,) and b["cldice_sums"].dtype == np.float64 and b["cldice_sums"].min() > 0
    assert b["cldice"] == float(cldice_from_sums(*[float(v) for v in b["cldice_sums"]], 1.0)) and 0.0 < b["cldice"] < 1.0
    assert b["objective"] == pytest.approx(a["objective"] + 0.5 * (1.0 - b["cldice"]), rel=1e-12)
