"""-m gpu: the Lovasz term (include/rsu_lovasz.h) through the C ABI. rsu_lovasz_fwd_bwd's gprob against hostio.lovasz_gradient BIT FOR
BIT from the identical float32 prob (the order is defined on bit patterns, every operation is rounded once), overwriting and accumulating;
loss_sum[0] against the mirror's losses within the bound of the two float32 summation orders (tests/lovasz_util.py), bit-identical
between runs; loss_sum[1] == B. Shapes: the issue's three and one below, at and above every boundary of the bitonic sort. Then the
argument errors and the network / model level above."""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from tests import cldice_util as CU  # noqa: E402
from tests import hiputil as hu  # noqa: E402
from tests import lovasz_util as LU  # noqa: E402
from tests.head_util import NETS, RSU_EINVAL, SMOOTH, _batch, _bits, _model, _net, _step  # noqa: E402
from road_segmentation_unet_amd import hostio  # noqa: E402
from road_segmentation_unet_amd._lib import RsuError, call, lib  # noqa: E402

# (shape, why it is here). The sort pads an image to Pn = max(4096, next power of two) keys, tiles of 4096 keys live in LDS, the merge
# steps of stride >= 4096 run through global memory up to three per launch, the scan and the sum work on tiles of 4096 ranks.
SHAPES = [
    ((1, 1, 1), "a single pixel: one key and 4095 of padding"),
    ((2, 5, 3), "odd and tiny, two images"),
    ((3, 37, 41), "the suite's usual odd shape: a third of a tile"),
    ((1, 63, 65), "4095 pixels: one short of the LDS tile"),
    ((1, 64, 64), "4096 pixels: exactly the LDS tile, no padding, no global step"),
    ((2, 17, 241), "4097 pixels: one over the tile -- two tiles per image, one global step (R = 1), a scan offset across tiles"),
    ((1, 1, 8191), "8191 pixels: one short of the padded power of two 8192"),
    ((1, 64, 128), "8192 pixels: exactly the padded power of two, both tiles full"),
    ((1, 3, 2731), "8193 pixels: one over -- Pn = 16384, the first stage with two global steps in one launch (R = 2)"),
    ((2, 128, 129), "16512 pixels: Pn = 32768, the first stage with three global steps in one launch (R = 3)"),
    ((2, 200, 201), "40200 pixels: Pn = 65536, the first stage that needs two global launches (R = 3, then R = 1)"),
]
BIG = ((1, 1025, 1024), "1 049 600 pixels: Pn = 2^21, 512 tiles per image -- the final sum's threads add more than one tile each")
KINDS = sorted(LU.INPUTS)


@functools.lru_cache(maxsize=None)
def _case(shape, kind):
    """(p, labels, mirror gradient, mirror losses): computed once per case and never written"""
    p, labels = LU.INPUTS[kind](shape)
    return p, labels, hostio.lovasz_gradient(p, labels, LU.SCALE), hostio.lovasz_loss(p, labels)


def _bufs(shape, p, labels, g0=None):
    return {"prob": hu.dev_f32(p), "labels": torch.from_numpy(labels).to(hu.DEV),
            "gprob": torch.full(shape, float("nan"), dtype=torch.float32, device=hu.DEV) if g0 is None else hu.dev_f32(g0),
            "loss": torch.zeros(2, dtype=torch.float32, device=hu.DEV),
            "ws": torch.full((LU.ws_bytes(shape) // 4,), -1, dtype=torch.int32, device=hu.DEV)}


def _check_loss(got, losses, shape, what):
    total = float(losses.astype(np.float64).sum())
    assert got[1] == shape[0], (what, got)
    if not np.isfinite(total):          # an infinity or a NaN among the errors: the same kind of non-finite result
        assert np.isnan(got[0]) == np.isnan(total) and (np.isnan(total) or got[0] == total), (what, got, total)
        return
    bound = LU.sum_bound(LU.host_depth(shape[1] * shape[2]) + LU.gpu_depth(shape), total)
    print("%s: loss_sum %.9g, mirror %.9g, |difference| %.3g, bound %.3g" % (what, got[0], total, abs(float(got[0]) - total), bound))
    assert abs(float(got[0]) - total) <= bound, (what, got, total, bound)


def _run_case(shape, kind):
    p, labels, g, losses = _case(shape, kind)
    what = "Lovasz %s %s" % (shape, kind)
    a = _bufs(shape, p, labels)
    LU.run_fwd_bwd(a, LU.SCALE, 0, shape, hu.stream())
    g0 = np.random.RandomState(11).standard_normal(shape).astype(np.float32)
    b = _bufs(shape, p, labels, g0)
    LU.run_fwd_bwd(b, LU.SCALE, 1, shape, hu.stream())
    torch.cuda.synchronize()
    got = a["gprob"].cpu().numpy()
    assert np.array_equal(got.view(np.uint32), g.view(np.uint32)), \
        (what, "overwriting: %d of %d pixels differ" % ((got.view(np.uint32) != g.view(np.uint32)).sum(), g.size))
    acc = b["gprob"].cpu().numpy()
    assert np.array_equal(acc.view(np.uint32), (g0 + g).view(np.uint32)), what + ": accumulating"
    la, lb = a["loss"].cpu().numpy(), b["loss"].cpu().numpy()
    _check_loss(la, losses, shape, what)
    assert np.array_equal(la.view(np.uint32), lb.view(np.uint32)), (what, "two runs", la, lb)
    counted = (labels == 0) | (labels == 1)
    if kind == "random" and counted.sum() > 100:
        # a match is no match of zeros (checked on the CPU for these inputs: above 0.9 at every shape)
        assert (g[counted] != 0).mean() > 0.5, (what, (g[counted] != 0).mean())
    ign = ~counted
    assert not got[ign].any() and not np.signbit(got[ign]).any(), what + ": +0 at ignored pixels"


@pytest.mark.parametrize("shape", [s for s, _ in SHAPES], ids=["%dx%dx%d" % s for s, _ in SHAPES])
def test_gradient_bits_and_loss(shape):
    assert LU.ws_bytes(shape) > 0
    for kind in KINDS:
        _run_case(shape, kind)


def test_more_than_256_tiles_per_image():
    _run_case(BIG[0], "random")


def test_forward_alone_adds_to_the_sums():
    shape = (3, 37, 41)
    p, labels, g, losses = _case(shape, "scattered_ignored")
    b = _bufs(shape, p, labels)
    LU.run_fwd(b, shape, hu.stream())
    torch.cuda.synchronize()
    once = b["loss"].clone()
    assert bool(torch.isnan(b["gprob"]).all())                  # the forward writes no gradient
    _check_loss(once.cpu().numpy(), losses, shape, "Lovasz forward")
    LU.run_fwd(b, shape, hu.stream())                           # on top of the first: += doubles (x + x is exact)
    LU.run_fwd_bwd(b, LU.SCALE, 0, shape, hu.stream())
    torch.cuda.synchronize()
    assert float(once[0]) > 0 and torch.equal(b["loss"], 3 * once)     # (2 x + x and 3 * x: one rounding each)
    assert float(b["loss"][1]) == 9.0
    assert np.array_equal(b["gprob"].cpu().numpy().view(np.uint32), g.view(np.uint32))


def test_the_tie_break_is_seen():
    """on the quantised map a sort that breaks ties the other way (descending index) gives another gradient at many pixels"""
    shape = (3, 37, 41)
    p, labels, g, _ = _case(shape, "quant4")
    other = hostio.lovasz_gradient(p[:, ::-1, ::-1], labels[:, ::-1, ::-1], LU.SCALE)[:, ::-1, ::-1]
    assert (other != g).mean() > 0.25


def test_argument_errors_leave_every_output_untouched():
    shape = (2, 9, 11)
    p, labels = LU.random_case(shape)
    b = _bufs(shape, p, labels, np.full(shape, 7.0, np.float32))
    b["loss"].fill_(7.0)
    L, P, st = lib(), hu.ptr, hu.stream()
    before = {n: b[n].clone() for n in ("gprob", "loss", "ws")}
    fwd = [P(b["prob"]), P(b["labels"]), P(b["loss"]), P(b["ws"]), 2, 9, 11, st]
    bwd = [P(b["prob"]), P(b["labels"]), 0.5, 0, P(b["gprob"]), P(b["loss"]), P(b["ws"]), 2, 9, 11, st]

    def bad(args, i, v):
        a = list(args)
        a[i] = v
        return a
    cases = [("rsu_lovasz_fwd", bad(fwd, i, None)) for i in (0, 1, 2, 3)]
    cases += [("rsu_lovasz_fwd", bad(fwd, i, v)) for i, v in ((4, 0), (5, 0), (6, 0), (4, -1), (4, 1 << 30), (5, 1 << 24))]
    cases += [("rsu_lovasz_fwd_bwd", bad(bwd, i, None)) for i in (0, 1, 4, 5, 6)]
    cases += [("rsu_lovasz_fwd_bwd", bad(bwd, i, v)) for i, v in ((7, 0), (8, 0), (9, -3), (7, 1 << 30), (9, 1 << 24))]
    cases += [("rsu_lovasz_fwd_bwd", bad(bwd, 2, v)) for v in (-1e-3, float("nan"), float("inf"), float("-inf"))]
    for name, args in cases:
        assert getattr(L, name)(*args) == RSU_EINVAL, (name, args)
    torch.cuda.synchronize()
    for n, t in before.items():
        assert torch.equal(_bits(b[n]), _bits(t)), n
    assert L.rsu_lovasz_fwd_bwd(*bad(bwd, 2, 0.0)) == 0          # scale == 0 is allowed: a gradient of zeros
    torch.cuda.synchronize()
    assert not bool(b["gprob"].any())


# ------------------------------------------------------------------------------------------- the network level
@pytest.mark.parametrize("L,root,dilated,P", NETS)
def test_net_without_the_term_is_the_default_net(L, root, dilated, P):
    a, b = _net(L, root, dilated, P), _net(L, root, dilated, P, lovasz_weight=0.0)
    assert b.lovasz_sum is None and b.gprob is None and b._lovasz_ws is None        # no buffer without the term
    outs = []
    for m in (a, b):
        _batch(m)
        outs.append(_step(m))
    for x, y in zip(*outs):
        assert torch.equal(_bits(x), _bits(y))
    c = _net(L, root, dilated, P, lovasz_weight=0.5)               # and the term switched off for one step
    _batch(c)
    for x, y in zip(outs[0], _step(c, lovasz_scale=0.0)):
        assert torch.equal(_bits(x), _bits(y))


def _aux(m, gprob, dice, focal, P, root):
    """rsu_head_fwd_bwd_aux on buffers of its own, fed `gprob`: (dact, dw, db, loss_sum)"""
    npix, C, p = m.B * P * P, root, hu.ptr
    z = lambda *s, dtype=torch.float32: torch.full(s, float("nan"), dtype=dtype, device=hu.DEV)  # noqa: E731
    prob, dsums, loss, wsum = z(npix), z(3), torch.zeros(1, device=hu.DEV), torch.zeros(1, device=hu.DEV)
    dact, dw, db = z(npix, C, dtype=torch.bfloat16), z(C, 2), z(2)
    ws = torch.zeros(lib().rsu_head_dice_ws_floats(npix, C), dtype=torch.float32, device=hu.DEV)
    head = (p(m.act[m.last_name]), p(m.w["weight_output/kernel"]), p(m.w["weight_output/bias"]))
    if dice:
        call("rsu_head_dice_sums", *head, p(m.labels), None, p(prob), p(dsums), p(ws), npix, C, hu.stream())
    call("rsu_head_fwd_bwd_aux", *head, p(m.labels), p(m._class_w_dev), None, focal, p(dsums) if dice else None, dice, SMOOTH, p(prob), p(loss),
         p(wsum), p(dact), p(dw), p(db), p(ws), npix, C, 1.0 / npix, p(gprob), hu.stream())
    torch.cuda.synchronize()
    return dact, dw, db, loss


@pytest.mark.parametrize("focal,dice", [(0.0, 0.0), (2.0, 0.7)], ids=["ce", "focal+dice"])
@pytest.mark.parametrize("L,root,dilated,P", NETS)
def test_net_gprob_is_the_mirror_of_its_prob(L, root, dilated, P, focal, dice):
    lam = 0.8
    m = _net(L, root, dilated, P, class_weights=(0.6, 2.5), dice_weight=dice, focal_gamma=focal, lovasz_weight=lam)
    _batch(m)
    m.labels.view(-1)[::7] = -1
    _step(m)
    prob, labels = m.prob.cpu().numpy(), m.labels.cpu().numpy()
    g = hostio.lovasz_gradient(prob, labels, lam)
    assert np.array_equal(m.gprob.cpu().numpy().view(np.uint32), g.view(np.uint32))
    # no match of zeros: a y = 1 pixel lowers I_k by one, so its g_k is never 0. (An untrained net's p is near 0.5 everywhere; where every
    # y = 1 pixel then ranks in front of every y = 0 pixel, I_k = 0 behind them and those g_k ARE 0, whatever the kernel does.)
    assert (g != 0).sum() >= (labels == 1).sum() > 100 and bool(np.all(g[labels == 1] < 0))
    losses = hostio.lovasz_loss(prob, labels)
    _check_loss(m.lovasz_sum.cpu().numpy(), losses, (m.B, P, P), "net lovasz_sum")
    dact, dw, db, loss = _aux(m, hu.dev_f32(g), dice, focal, P, root)
    npix = m.B * P * P
    for name, got, ref in (("dact", m.grad[m.last_name].reshape(npix, root), dact), ("dw", m.g["weight_output/kernel"].reshape(root, 2), dw),
                           ("db", m.g["weight_output/bias"], db), ("loss_sum", m.loss_sum, loss)):
        assert torch.equal(_bits(got), _bits(ref)), name
    # the term reaches the whole net's gradient
    g1 = m.flat_g.clone()
    _step(m, lovasz_scale=0.0)
    assert float((g1 - m.flat_g).abs().max()) > 1e-3 * float(m.flat_g.abs().max())
    # the evaluation pass adds the same sums to its own accumulator
    m.reset_eval()
    m.forward_device(keep=1.0)
    m.evaluate_device()
    m.evaluate_device()
    torch.cuda.synchronize()
    ev = m.eval_lovasz_sum.cpu().numpy()
    ev_losses = hostio.lovasz_loss(m.prob.cpu().numpy(), labels)
    assert ev[1] == 2 * m.B
    _check_loss(np.array([ev[0] / 2, m.B], np.float32), ev_losses, (m.B, P, P), "net eval_lovasz_sum")
    m.reset_eval()
    assert not bool(m.eval_lovasz_sum.any())


@pytest.mark.parametrize("L,root,dilated,P", NETS)
def test_net_adds_the_term_to_the_cldice_gradient(L, root, dilated, P):
    lam, cl, iters = 0.8, 0.6, 3
    m = _net(L, root, dilated, P, cldice_weight=cl, cldice_iters=iters, lovasz_weight=lam)
    _batch(m)
    m.labels.view(-1)[::7] = -1
    _step(m)
    shape = (m.B, P, P)
    prob, labels = m.prob.cpu().numpy(), m.labels.cpu().numpy()
    z = lambda *s: torch.full(s, float("nan"), dtype=torch.float32, device=hu.DEV)  # noqa: E731
    o = {"prob": m.prob, "labels": m.labels, "skel_p": z(*shape), "skel_y": z(*shape), "gprob": z(*shape),
         "sums": torch.zeros(4, dtype=torch.float32, device=hu.DEV), "ws": z(CU.ws_floats(shape, iters))}
    CU.run_fwd(o, iters, shape, hu.stream())
    CU.run_bwd(o, iters, cl, 1.0, shape, hu.stream())
    torch.cuda.synchronize()
    g_cl = o["gprob"].cpu().numpy()
    want = hostio.lovasz_gradient(prob, labels, lam, into=g_cl)      # one rounding on top of the clDice entry's own gradient
    assert np.array_equal(m.gprob.cpu().numpy().view(np.uint32), want.view(np.uint32))
    host_cl = hostio.cldice_gradient(prob, labels, iters, cl, 1.0)[3]
    hu.assert_f32_close(m.gprob.cpu().numpy(), host_cl + hostio.lovasz_gradient(prob, labels, lam).astype(np.float64), "clDice + Lovasz gprob")
    assert bool(torch.any(o["gprob"] != 0)) and float(m.cldice_sums.min()) > 0


def test_net_refuses_bad_values():
    L, root, dilated, P = NETS[1]
    for kw in ({"lovasz_weight": -1.0}, {"lovasz_weight": float("nan")}, {"lovasz_weight": "x"}):
        with pytest.raises(RsuError):
            _net(L, root, dilated, P, **kw)
    from road_segmentation_unet_amd.unet import UNet
    with pytest.raises(RsuError):
        UNet(L, root, dilated, 2, P, seed=17, training=False, lovasz_weight=1.0)
    m = _net(L, root, dilated, P, lovasz_weight=0.5)
    _batch(m)
    m.forward_device()
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(RsuError):
            m.backward_device(1.0 / (m.B * P * P), lovasz_scale=bad)
    with pytest.raises(RsuError):
        m.lovasz_weight = -1
    assert m.lovasz_weight == 0.5


# ------------------------------------------------------------------------------------------- the model level
def _stripes(m):
    """the batch of tests/test_gpu_cldice.py::test_model_trains_with_the_cldice_term"""
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


def test_model_reports_the_loss_with_the_term():
    """ten steps on the stripes batch at lambda = 1: the logged loss is cross-entropy + the mean per-image Lovasz loss of the step's prob"""
    m = _model(lovasz_weight=1.0)
    assert m.net.lovasz_weight == 1.0
    X, y = _stripes(m)
    losses = []
    for step in range(10):
        loss, prob = m.train_step(X, y)
        pr = prob.cpu().numpy()
        lv = float(hostio.lovasz_loss(pr, y).astype(np.float64).mean())
        p1 = pr.astype(np.float64)
        ce = float(-np.log(np.where(y == 1, p1, 1.0 - p1)).mean())
        got = float(loss)
        print("step %2d: loss %.7f host %.7f  lovasz %.5f" % (step, got, ce + lv, lv))
        assert abs(got - (ce + lv)) <= 1e-5 * max(1.0, abs(got)), (step, got, ce, lv)
        losses.append(got)
    assert losses[-1] < losses[0] and bool(torch.all(torch.isfinite(m.net.flat_w)))


def test_evaluate_reports_lovasz():
    plain, m = _model(), _model(lovasz_weight=0.5)
    X, y = _stripes(m)
    X, y = np.concatenate([X, X[::-1]])[:3], np.concatenate([y, y[::-1]])[:3]   # three patches at a batch of two: the last chunk is padded
    a, b = plain.evaluate(X, y), m.evaluate(X, y)
    assert "lovasz" not in a
    for k in a:
        if k != "objective":
            assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    # the host figure: the per-image mirror losses of the probabilities the two chunks leave in net.prob
    per = []
    for lo, hi in ((0, 2), (2, 3)):
        m.evaluate(X[lo:hi], y[lo:hi])
        per += list(hostio.lovasz_loss(m.net.prob.cpu().numpy()[:hi - lo], y[lo:hi]).astype(np.float64))
    want = float(np.mean(per))
    assert 0.0 < want < 1.0 and abs(b["lovasz"] - want) <= 1e-5 * want, (b["lovasz"], want)
    assert b["objective"] == pytest.approx(a["objective"] + 0.5 * b["lovasz"], rel=1e-12)
