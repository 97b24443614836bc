"""-m gpu: held-out validation. The evaluation head (rsu.h rsu_head_eval) through the C ABI against float64 torch built from the same
bf16-rounded inputs (tests/test_gpu_dice_loss.py's inputs and reference), bit for bit against the training heads it shares its mapping
with, its histogram against a numpy restatement from the returned prob; then UNet.evaluate_device / ConvolutionalModel.evaluate above it:
padding exactness, freedom from side effects on training, two ranks against one. Tolerances: the hiputil defaults for prob, 2e-5 relative
for head scalar sums (tests/test_gpu_dice_loss.py, tests/test_gpu_weighted_loss.py), the net-level ones of tests/test_gpu_net.py."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

pytestmark = pytest.mark.gpu

from oracle import unet_oracle as U  # noqa: E402
from tests import hiputil as hu  # noqa: E402
from tests.head_util import NPIX, Ref, _bits, _dev_labels, _inputs, _weight_map, _with_ignored  # noqa: E402
from road_segmentation_unet_amd._lib import EVAL_BINS, call, lib  # noqa: E402

RSU_EINVAL = -22   # include/rsu.h
BINS = 256
CS = [64, 16]
CW = (0.6, 2.5)


class EvalOut:
    def __init__(self, C, npix=NPIX, fill=0.0):
        z = lambda *s, dtype=torch.float32: torch.full(s, fill, dtype=dtype, device=hu.DEV)  # noqa: E731
        self.prob, self.sums = z(npix), z(5)
        self.hist = torch.full((2, BINS), int(fill), dtype=torch.int64, device=hu.DEV)
        self.ws = z(int(lib().rsu_head_eval_ws_floats(npix, C)))
        # buffers no argument points at: what the training heads would write (dact, dw, db, loss_sum / weight_sum, dice_sums)
        self.others = [("dact", z(npix, C, dtype=torch.bfloat16)), ("dw", z(C, 2)), ("db", z(2)), ("loss_acc", z(2)), ("dice_sums", z(3))]


def _eval(C, act_d, w_d, b_d, labels, class_w, pixel_w, o=None, npix=NPIX, times=1):
    o = o or EvalOut(C, npix)
    lab = labels if torch.is_tensor(labels) else _dev_labels(labels)
    cw = hu.dev_f32(np.asarray(class_w, np.float32)) if class_w is not None else None
    pw = pixel_w if (pixel_w is None or torch.is_tensor(pixel_w)) else hu.dev_f32(pixel_w)
    for _ in range(times):
        call("rsu_head_eval", hu.ptr(act_d), hu.ptr(w_d), hu.ptr(b_d), hu.ptr(lab), hu.ptr(cw), hu.ptr(pw), hu.ptr(o.prob), hu.ptr(o.sums),
             hu.ptr(o.hist), hu.ptr(o.ws), npix, C, hu.stream())
    torch.cuda.synchronize()
    return o


def _hist_from_prob(prob, labels):
    """the numpy restatement: exact, because the multiplication by 256 is exact in f32"""
    prob = np.asarray(prob, np.float32)
    bins = np.minimum(BINS - 1, (prob * np.float32(BINS)).astype(np.int64))
    return np.stack([np.bincount(bins[labels == l], minlength=BINS) for l in (0, 1)]).astype(np.int64)


def _case(C, mode, scale=1.0):
    """(act, w, b, labels, class_w, pixel_w) of the four combinations the head must serve"""
    rng, act, w, b, labels = _inputs(C)
    w = (w * np.float32(scale)).astype(np.float32)
    class_w = CW if mode in ("class", "ignored") else None
    pixel_w = _weight_map(rng) if mode in ("map", "ignored") else None
    if mode == "ignored":
        labels, ign = _with_ignored(rng, labels)
        assert (labels == 2 ** 32 + 1).sum() == 1
        pixel_w[np.nonzero(ign)[0][:3]] = [np.inf, np.nan, -1e30]     # never multiplied: ignored by selection
    return act, w, b, labels, class_w, pixel_w


MODES = ["plain", "class", "map", "ignored"]


def test_abi_constant():
    assert EVAL_BINS == BINS


# ------------------------------------------------------------------------------------------- the op against float64
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("mode", MODES)
def test_eval_head_against_float64(C, mode):
    act, w, b, labels, class_w, pixel_w = _case(C, mode)
    o = _eval(C, hu.dev_bf16(act), hu.dev_f32(w), hu.dev_f32(b), labels, class_w, pixel_w)
    safe_pw = None if pixel_w is None else np.where((labels == 0) | (labels == 1), pixel_w, 1.0)
    ref = Ref(act, w, b, labels, class_w, safe_pw, 1.0 / NPIX, lam=0.0)
    hu.assert_f32_close(hu.host(o.prob), ref.prob, "eval prob (%s, C=%d)" % (mode, C))
    got = o.sums.cpu().numpy().astype(np.float64)
    want = np.array([ref.ce_sum, ref.wsum, ref.sums[0], ref.sums[1], ref.sums[2]])
    print("eval sums (%s, C=%d): got %s ref %s" % (mode, C, got, want))
    for g, r, n in zip(got, want, ("omega CE", "omega", "I", "P", "Y")):
        assert r > 1.0, (n, r)                            # (no sum is near zero: the relative bound means something)
        assert abs(g - r) <= 2e-5 * abs(r), (mode, C, n, g, r)
    if mode in ("map", "ignored"):
        assert (pixel_w == 0).sum() > 0
    # the histogram: exactly the restatement from the returned prob, over the counted pixels whatever their weights are
    h = o.hist.cpu().numpy()
    counted = (labels == 0) | (labels == 1)
    assert np.array_equal(h, _hist_from_prob(o.prob.cpu().numpy(), labels)), (mode, C)
    assert int(h.sum()) == int(counted.sum()) and int(h[1].sum()) == int((labels == 1).sum())
    if mode == "ignored":
        assert int(counted.sum()) < NPIX


# ------------------------------------------------------------------------------------------- the op against its siblings, bit for bit
@pytest.mark.parametrize("C", CS)
@pytest.mark.parametrize("mode", MODES)
def test_eval_head_has_the_training_heads_bits(C, mode):
    act, w, b, labels, class_w, pixel_w = _case(C, mode)
    ad, wd, bd, lab = hu.dev_bf16(act), hu.dev_f32(w), hu.dev_f32(b), _dev_labels(labels)
    cw = hu.dev_f32(np.asarray(class_w, np.float32)) if class_w is not None else None
    pw = hu.dev_f32(pixel_w) if pixel_w is not None else None
    o = _eval(C, ad, wd, bd, lab, class_w, pw)
    z = lambda *s, dtype=torch.float32: torch.zeros(s, dtype=dtype, device=hu.DEV)  # noqa: E731
    prob_w, prob_d, acc, dsums = z(NPIX), z(NPIX), z(2), z(3)
    dact, dw, db = z(NPIX, C, dtype=torch.bfloat16), z(C, 2), z(2)
    ws = z(int(lib().rsu_head_dice_ws_floats(NPIX, C)))
    call("rsu_head_fwd_bwd_w", hu.ptr(ad), hu.ptr(wd), hu.ptr(bd), hu.ptr(lab), hu.ptr(cw), hu.ptr(pw), hu.ptr(prob_w), hu.ptr(acc[0:1]),
         hu.ptr(acc[1:2]), hu.ptr(dact), hu.ptr(dw), hu.ptr(db), hu.ptr(ws), NPIX, C, 1.0 / NPIX, hu.stream())
    call("rsu_head_dice_sums", hu.ptr(ad), hu.ptr(wd), hu.ptr(bd), hu.ptr(lab), hu.ptr(pw), hu.ptr(prob_d), hu.ptr(dsums), hu.ptr(ws), NPIX, C,
         hu.stream())
    torch.cuda.synchronize()
    print("eval %s | fwd_bwd_w %s | dice_sums %s" % (o.sums.cpu().tolist(), acc.cpu().tolist(), dsums.cpu().tolist()))
    assert torch.equal(_bits(o.prob), _bits(prob_d)) and torch.equal(_bits(o.prob), _bits(prob_w)), "prob"
    assert torch.equal(_bits(o.sums[0:2]), _bits(acc)), "sums[0..1] vs loss_sum, weight_sum"
    assert torch.equal(_bits(o.sums[2:5]), _bits(dsums)), "sums[2..4] vs {I, P, Y}"
    assert bool(torch.all(torch.isfinite(o.sums)))


# ------------------------------------------------------------------------------------------- saturated probabilities
@pytest.mark.parametrize("C,npix", [(64, NPIX), (16, NPIX), (64, 4 * 388 * 388)])
def test_histogram_of_saturated_probabilities(C, npix):
    """w x 40: nearly every pixel lands in bin 0 or bin 255 -- every block's counts meet on two addresses"""
    if npix == NPIX:
        act, w, b, labels, class_w, pixel_w = _case(C, "ignored", scale=40.0)
        z = act.astype(np.float64) @ w.astype(np.float64) + b.astype(np.float64)
        ad, wd, bd, lab, pw = hu.dev_bf16(act), hu.dev_f32(w), hu.dev_f32(b), _dev_labels(labels), hu.dev_f32(pixel_w)
    else:   # the c2 head geometry, 1024 blocks
        gen = torch.Generator(device="cpu").manual_seed(C + npix)
        a32 = torch.relu(torch.randn((npix, C), generator=gen)).to(torch.bfloat16)
        w32, b32 = 40.0 * 0.3 * torch.randn((C, 2), generator=gen), 0.1 * torch.randn(2, generator=gen)
        z = (a32.to(torch.float64) @ w32.to(torch.float64) + b32.to(torch.float64)).numpy()
        labels = (torch.rand(npix, generator=gen) < 0.2).to(torch.int64)
        labels[torch.rand(npix, generator=gen) < 0.05] = -1
        labels = labels.numpy()
        ad, wd, bd, lab, pw = a32.to(hu.DEV), w32.to(hu.DEV), b32.to(hu.DEV), _dev_labels(labels), None
    p_ref = 1.0 / (1.0 + np.exp(np.clip(z[:, 0] - z[:, 1], -700.0, 700.0)))                      # the CPU reference
    at_ends = float(((p_ref < 1.0 / BINS) | (p_ref >= (BINS - 1.0) / BINS)).mean())
    print("C %d npix %d: %.2f %% of the reference probabilities in bins 0 and 255" % (C, npix, 100 * at_ends))
    assert at_ends >= 0.90
    o = _eval(C, ad, wd, bd, lab, CW, pw, npix=npix)
    hu.assert_f32_close(hu.host(o.prob), p_ref, "saturated prob")
    h = o.hist.cpu().numpy()
    assert np.array_equal(h, _hist_from_prob(o.prob.cpu().numpy(), labels))
    assert int(h.sum()) == int(((labels == 0) | (labels == 1)).sum())
    assert int(h[:, 0].sum() + h[:, -1].sum()) >= 0.85 * int(h.sum())
    again = _eval(C, ad, wd, bd, lab, CW, pw, npix=npix)
    assert torch.equal(o.hist, again.hist) and torch.equal(_bits(o.sums), _bits(again.sums)) and torch.equal(_bits(o.prob), _bits(again.prob))


# ------------------------------------------------------------------------------------------- accumulation, determinism, untouched memory
@pytest.mark.parametrize("C", CS)
def test_eval_head_accumulates_and_is_deterministic(C):
    act, w, b, labels, class_w, pixel_w = _case(C, "ignored")
    ad, wd, bd, lab, pw = hu.dev_bf16(act), hu.dev_f32(w), hu.dev_f32(b), _dev_labels(labels), hu.dev_f32(pixel_w)
    one = _eval(C, ad, wd, bd, lab, class_w, pw)
    two = _eval(C, ad, wd, bd, lab, class_w, pw, times=2)
    assert torch.equal(two.hist, 2 * one.hist) and int(one.hist.sum()) > 0
    assert torch.equal(_bits(two.sums), _bits(one.sums + one.sums)), "x + x in f32"
    fresh = _eval(C, ad, wd, bd, lab, class_w, pw)
    assert torch.equal(fresh.hist, one.hist) and torch.equal(_bits(fresh.sums), _bits(one.sums)) and torch.equal(_bits(fresh.prob), _bits(one.prob))
    # accumulators that start from something else than zero keep it
    o = EvalOut(C, fill=3.0)
    _eval(C, ad, wd, bd, lab, class_w, pw, o=o)
    assert torch.equal(o.hist, one.hist + 3) and torch.equal(_bits(o.sums), _bits(one.sums + 3.0))
    for name, t in o.others:
        assert bool(torch.all(t == 3.0)), "%s: no argument points at it" % name


def test_eval_head_argument_checks():
    C = 16
    _, act, w, b, labels = _inputs(C)
    ad, wd, bd, lab = hu.dev_bf16(act), hu.dev_f32(w), hu.dev_f32(b), _dev_labels(labels)
    o = EvalOut(C, fill=7.0)
    assert lib().rsu_head_eval_ws_floats(NPIX, C) > 0 and lib().rsu_head_eval_ws_floats(NPIX, 12) == 0 and lib().rsu_head_eval_ws_floats(0, C) == 0

    def rc(act=ad, w=wd, b=bd, labels=lab, prob=o.prob, sums=o.sums, hist=o.hist, ws=o.ws, C=C, npix=NPIX):
        return lib().rsu_head_eval(hu.ptr(act), hu.ptr(w), hu.ptr(b), hu.ptr(labels), None, None, hu.ptr(prob), hu.ptr(sums), hu.ptr(hist),
                                   hu.ptr(ws), npix, C, hu.stream())
    for name in ("act", "w", "b", "labels", "prob", "sums", "hist", "ws"):
        assert rc(**{name: None}) == RSU_EINVAL, name
    for bad_c in (0, 12, 24, 520):
        assert rc(C=bad_c) == RSU_EINVAL, bad_c
    assert rc(npix=0) == RSU_EINVAL and rc(npix=-5) == RSU_EINVAL
    torch.cuda.synchronize()
    for name, t in [("prob", o.prob), ("sums", o.sums), ("hist", o.hist), ("ws", o.ws)] + o.others:
        assert bool(torch.all(t == 7)), "%s was written by a refused call" % name
    assert rc() == 0          # class_w and pixel_w may be NULL
    torch.cuda.synchronize()
    assert int(o.hist.sum()) == 7 * 2 * BINS + NPIX


# ------------------------------------------------------------------------------------------- the network and the model
ML, MROOT, MP, MB = 3, 16, 20, 2      # the small config of the other model tests


def _model(**kw):
    from road_segmentation_unet_amd.model import ConvolutionalModel, Options
    o = dict(num_layers=ML, root_size=MROOT, patch_size=MP, batch_size=MB, dilated_layers=True, dropout=1.0, lr=0.01, seed=5, logdir=None)
    o.update(kw)
    return ConvolutionalModel(Options(**o), device="cuda:0", params=U.init_params(ML, MROOT, True, seed=13, bias_scale=0.05))


def _patches(n, seed=21, p_road=0.3):
    S = U.input_size_needed(MP, ML)
    rng = np.random.RandomState(seed)
    return rng.rand(n, S, S, 3).astype(np.float32), (rng.rand(n, MP, MP) < p_road).astype(np.int64)


def _abi_accumulate(m, X, y, weights=None):
    """what evaluate() is specified to do, restated through the ABI: per batch a forward pass and ONE rsu_head_eval on the net's last
    activation, into accumulators of the test's own; the last batch padded with zero patches labelled -1"""
    net, B = m.net, m.local_batch
    sums = torch.zeros(5, dtype=torch.float32, device=hu.DEV)
    hist = torch.zeros((2, BINS), dtype=torch.int64, device=hu.DEV)
    prob = torch.zeros((B, MP, MP), dtype=torch.float32, device=hu.DEV)
    ws = torch.zeros(int(lib().rsu_head_eval_ws_floats(B * MP * MP, MROOT)), dtype=torch.float32, device=hu.DEV)
    cw = net._class_w_dev
    for t0 in range(0, len(X), B):
        nb = min(B, len(X) - t0)
        xb, yb = np.zeros((B,) + X.shape[1:], np.float32), np.full((B, MP, MP), -1, np.int64)
        xb[:nb], yb[:nb] = X[t0:t0 + nb], y[t0:t0 + nb]
        net.x.copy_(torch.from_numpy(xb))
        net.labels.copy_(torch.from_numpy(yb))
        pw = None
        if weights is not None:
            wb = np.ones((B, MP, MP), np.float32)
            wb[:nb] = weights[t0:t0 + nb]
            pw = hu.dev_f32(wb)
        net.forward_device(keep=1.0)
        call("rsu_head_eval", hu.ptr(net.act[net.last_name]), hu.ptr(net.w["weight_output/kernel"]), hu.ptr(net.w["weight_output/bias"]),
             hu.ptr(net.labels), hu.ptr(cw), hu.ptr(pw), hu.ptr(prob), hu.ptr(sums), hu.ptr(hist), hu.ptr(ws), B * MP * MP, MROOT, hu.stream())
    torch.cuda.synchronize()
    return sums.cpu().numpy().astype(np.float64), hist.cpu().numpy(), prob.cpu().numpy()


@pytest.mark.parametrize("with_map", [False, True])
def test_model_evaluate_equals_the_abi_and_the_oracle(with_map):
    from road_segmentation_unet_amd.model import dice_from_sums, metrics_from_eval
    lam, N = 0.7, 5
    m = _model(class_weights=CW, dice_weight=lam)
    X, y = _patches(N)
    weights = (0.25 + np.random.RandomState(8).rand(N, MP, MP)).astype(np.float32) if with_map else None
    assert N % m.local_batch != 0
    assert tuple(m.net.eval_sums.shape) == (5,) and tuple(m.net.eval_hist.shape) == (2, BINS) and m.net.eval_hist.dtype == torch.int64
    assert "eval_sums" not in m.net.state_dict() and "eval_hist" not in m.net.state_dict()
    out = m.evaluate(X, y, weights=weights, threshold=0.5)
    sums, hist, last_prob = _abi_accumulate(m, X, y, weights)
    assert np.array_equal(out["hist"], hist) and int(hist.sum()) == N * MP * MP
    assert np.array_equal(out["sums"], sums), (out["sums"], sums)
    want = metrics_from_eval(sums, hist, N * MP * MP, lam, 1.0, 0.5)
    for k, v in want.items():
        assert out[k] == v, k
    nl = N % m.local_batch
    assert np.array_equal(m.net.prob.cpu().numpy()[:nl], last_prob[:nl])         # net.prob: the last chunk's probabilities
    # the float64 restatement over the bf16-emulating oracle's probabilities of the same patches
    params = U.init_params(ML, MROOT, True, seed=13, bias_scale=0.05)         # (_model's)
    p = np.concatenate([U.predict_probs(params, X[i:i + 1], ML, MROOT, True, emulate_bf16=True) for i in range(N)])
    p = p.astype(np.float64).reshape(N, MP, MP)
    assert float(np.abs(last_prob[:nl] - p[N - nl:]).max()) <= 4e-3
    pw = np.ones((N, MP, MP)) if weights is None else weights.astype(np.float64)
    ce = -np.where(y == 1, np.log(p), np.log1p(-p))
    omega = np.where(y == 1, CW[1], CW[0]) * pw
    rloss = float((omega * ce).sum()) / (N * MP * MP)
    print("evaluate: loss %.7f oracle %.7f; weighted mean %.7f; dice %.5f; f1 %.4f best %.4f at %.4f"
          % (out["loss"], rloss, out["weighted_mean_loss"], out["dice"], out["f1"], out["best_f1"], out["best_threshold"]))
    assert abs(out["loss"] - rloss) <= 2e-3 * abs(rloss), (out["loss"], rloss)                      # tests/test_gpu_net.py's rule
    assert abs(out["weighted_mean_loss"] - float((omega * ce).sum() / omega.sum())) <= 2e-3 * abs(rloss)
    I, P, Y = float((pw * p * y).sum()), float((pw * p).sum()), float((pw * y).sum())
    D = dice_from_sums(I, P, Y, 1.0)
    bound = 4e-3 * (2.0 * Y + pw.sum()) / (P + Y + 1.0)      # every probability within 4e-3: |dD| <= (2 dI + D dP) / U, D <= 1
    assert abs(out["dice"] - D) <= bound, (out["dice"], D, bound)
    assert out["objective"] == out["loss"] + lam * (1.0 - out["dice"])
    # the counts at 0.5 against the oracle's probabilities: only pixels within the probability tolerance of the threshold may differ
    near = int((np.abs(p - 0.5) <= 4e-3).sum())
    tp_ref = int(((p >= 0.5) & (y == 1)).sum())
    assert abs(out["tp"] - tp_ref) <= near and out["tp"] + out["fn"] == int((y == 1).sum()) and out["fp"] + out["tn"] == int((y == 0).sum())
    with pytest.raises(ValueError):
        m.evaluate(X, y, threshold=0.3)


def test_model_evaluate_padding_is_exact():
    m = _model(class_weights=CW, dice_weight=0.7)
    N, B = 7, 2
    X, y = _patches(N, seed=22)
    y[1, :4] = -1                                             # ignored pixels inside real patches count in n_pixels, not in the histogram
    whole = m.evaluate(X, y)
    head, tail = m.evaluate(X[:N - N % B], y[:N - N % B]), m.evaluate(X[N - N % B:], y[N - N % B:])
    assert np.array_equal(whole["hist"], head["hist"] + tail["hist"])
    assert int(whole["hist"].sum()) == N * MP * MP - 4 * MP and whole["n_pixels"] == N * MP * MP
    for a, b, c in zip(whole["sums"], head["sums"], tail["sums"]):
        assert abs(a - (b + c)) <= 2e-5 * abs(a), (a, b, c)
    assert np.array_equal(m.evaluate(X, y)["hist"], whole["hist"]) and np.array_equal(m.evaluate(X, y)["sums"], whole["sums"])


@pytest.mark.parametrize("optimizer", ["adam", "momentum"])
def test_evaluate_leaves_training_untouched(optimizer):
    """3 steps with dropout 0.8, twice from the same seed, once with evaluate() in front of and between the steps"""
    Xs, ys = _patches(3 * MB, seed=23)
    Xv, yv = _patches(3, seed=24)
    wmap = (0.5 + np.random.RandomState(9).rand(MB, MP, MP)).astype(np.float32)
    vmap = (0.25 + np.random.RandomState(10).rand(3, MP, MP)).astype(np.float32)

    def run(with_eval):
        m = _model(optimizer=optimizer, dropout=0.8, class_weights=CW, dice_weight=0.3, lr=0.01 if optimizer == "momentum" else 0.001)
        losses = []
        for k in range(3):
            if with_eval:
                g0, step0 = m.net.flat_g.clone(), m.net.global_step
                x0, l0 = m.net.x.clone(), m.net.labels.clone()
                pw0 = None if m.net.pixel_weights is None else m.net.pixel_weights.clone()
                keys0 = [m.net.dropout_key(s) for s in range(2 * ML - 1)]
                v = m.evaluate(Xv, yv, weights=vmap if k == 1 else None)
                assert v["n_counted"] == 3 * MP * MP and v["loss"] > 0
                assert torch.equal(_bits(m.net.flat_g), _bits(g0)) and m.net.global_step == step0
                assert torch.equal(m.net.x, x0) and torch.equal(m.net.labels, l0)
                assert (pw0 is None and m.net.pixel_weights is None) or torch.equal(m.net.pixel_weights, pw0)
                assert [m.net.dropout_key(s) for s in range(2 * ML - 1)] == keys0
            loss, _ = m.train_step(Xs[k * MB:(k + 1) * MB], ys[k * MB:(k + 1) * MB], weights=wmap if k != 1 else None)
            losses.append(loss.clone())
        torch.cuda.synchronize()
        slots = [m.net.flat_acc.clone()] + ([m.net.flat_v.clone()] if optimizer == "adam" else [])
        return m.net.flat_w.clone(), slots, m.net.global_step, losses

    w_a, s_a, step_a, loss_a = run(True)
    w_b, s_b, step_b, loss_b = run(False)
    assert step_a == step_b == 3
    assert torch.equal(_bits(w_a), _bits(w_b)), "weights"
    assert len(s_a) == len(s_b) == (2 if optimizer == "adam" else 1)
    for a, b in zip(s_a, s_b):
        assert torch.equal(_bits(a), _bits(b)), "optimizer slots"
    for a, b in zip(loss_a, loss_b):
        assert torch.equal(_bits(a), _bits(b)), "loss"
    w0 = torch.from_numpy(np.concatenate([v.reshape(-1) for v in U.init_params(ML, MROOT, True, seed=13, bias_scale=0.05).values()]))
    assert w_a.numel() >= w0.numel() and float(loss_a[-1]) > 0 and bool(torch.all(torch.isfinite(w_a)))
    assert bool(torch.any(s_a[0] != 0)), "the steps did step"


def test_train_loop_validates_and_keeps_the_best(tmp_path):
    import json
    Xs, ys = _patches(9, seed=25)
    Xv, yv = _patches(3, seed=26)
    m = _model(validate_every=2, save_best=True, save_path=str(tmp_path / "runs"), logdir=str(tmp_path / "log"))
    st = m.train(Xs, ys.astype(np.float64), None, None)
    assert "validation" not in st                                                    # off by default: nothing ran
    st = m.train(Xs, ys.astype(np.float64), None, None, validation=(Xv, yv))
    assert st["patches"] == 8 and set(("loss", "objective", "dice", "f1", "iou", "best_threshold")) <= set(st["validation"])
    assert m.best_val_f1 is not None and os.path.exists(str(tmp_path / "runs" / (m.experiment_name + "-best.chkpt.npz")))
    rows = [json.loads(l) for l in open(os.path.join(str(tmp_path / "log"), m.experiment_name, "events.jsonl"))]
    tags = {}
    for r in rows:
        tags.setdefault(r["tag"], []).append(r["step"])
    for t in ("val_loss", "val_objective", "val_dice", "val_f1", "val_iou", "val_best_threshold"):
        assert tags[t] == [6, 8], (t, tags.get(t))                                   # steps 5..8 of the second epoch, every 2
    m2 = _model(validate_every=0, logdir=None)
    st = m2.train(Xs, ys.astype(np.float64), None, None, validation=(Xv, yv))
    assert st["validation"]["n_pixels"] == 3 * MP * MP


# ------------------------------------------------------------------------------------------- two ranks on one GPU
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LOCAL_RANK="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        m = _model(batch_size=2 * MB, class_weights=CW, dice_weight=0.7)
        assert m.world == world and m.local_batch == MB
        X, y = _patches(7, seed=27)
        out = m.evaluate(X, y)
        q.put((rank, out["sums"], out["hist"], out["f1"], out["loss"]))
    finally:
        dist.destroy_process_group()


def test_two_rank_evaluate_equals_one_rank():
    X, y = _patches(7, seed=27)
    ref = _model(batch_size=MB, class_weights=CW, dice_weight=0.7).evaluate(X, y)
    torch.cuda.synchronize()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(2)]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    assert sorted(r[0] for r in res) == [0, 1]
    for _, sums, hist, f1, loss in res:
        assert np.array_equal(hist, ref["hist"])
        for a, b in zip(sums, ref["sums"]):
            assert abs(a - b) <= 2e-5 * abs(b), (sums, ref["sums"])
        assert f1 == ref["f1"] and abs(loss - ref["loss"]) <= 2e-5 * abs(ref["loss"])
    assert np.array_equal(res[0][1], res[1][1])          # both ranks hold the same reduced sums
