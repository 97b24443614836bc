"""-m gpu: the exponential moving average of the weights -- the device pass (rsu_ema_step) bit for bit against its numpy float32
restatement, over repeated calls and under a skipped step's record; the averaging net beside a twin without averaging (training is not
perturbed, the averages follow the host recurrence); averaged_weights(); checkpoints; ConvolutionalModel and the command line.
Every comparison is bit equality: against the float32 restatement, or against the project's own plain path."""
import os
import re

import numpy as np
import pytest
import torch

from road_segmentation_unet_amd import _lib
from road_segmentation_unet_amd._lib import RsuError, call
from road_segmentation_unet_amd.unet import EMA_SUFFIX, UNet, ema_decay_at, param_shapes

pytestmark = pytest.mark.gpu

f32 = np.float32
DEV = "cuda:0"
PAD = 64                                   # floats in front of and behind a slice: 256 bytes, so the slice stays 16-byte aligned
SHARE = 8192                               # floats per workgroup of the pass (rsu.h)
NS = [1, 3, 4, 5, 1023, 1024, SHARE, SHARE + 5, 16384 + 7, 3 * 16384 + 1]
OMDS = [1.0, 0.25, 2.0 ** -10, 1e-4]


def _stream():
    return torch.cuda.current_stream().cuda_stream


def host_ema(e, w, omd):
    """the pass restated in numpy float32: three roundings per element, in the kernel's order"""
    e, w, omd = np.asarray(e, f32), np.asarray(w, f32), f32(omd)
    d = (e - w).astype(f32)
    return (e - (d * omd).astype(f32)).astype(f32)


def bits(t):
    a = t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def same(a, b):
    return np.array_equal(bits(a), bits(b))


class Slices:
    """ema[0:n) and w[0:n) as slices of two larger buffers of random floats"""

    def __init__(self, n, seed):
        rng = np.random.RandomState(seed)
        self.n = n
        self.big_e = torch.from_numpy(rng.randn(n + 2 * PAD).astype(f32)).to(DEV)
        self.big_w = torch.from_numpy(rng.randn(n + 2 * PAD).astype(f32)).to(DEV)
        self.e, self.w = self.big_e[PAD:PAD + n], self.big_w[PAD:PAD + n]
        assert self.e.data_ptr() % 16 == 0 and self.w.data_ptr() % 16 == 0

    def run(self, omd, record=None):
        call("rsu_ema_step", self.e.data_ptr(), self.w.data_ptr(), self.n, float(f32(omd)), None if record is None else record.data_ptr(), _stream())
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- 1. the kernel
@pytest.mark.parametrize("omd", OMDS)
@pytest.mark.parametrize("n", NS)
def test_pass_equals_the_float32_restatement(n, omd):
    s = Slices(n, 100 + n % 991)
    e0, w0 = s.big_e.cpu().numpy().copy(), s.big_w.cpu().numpy().copy()
    s.run(omd)
    e1 = s.big_e.cpu().numpy()
    assert same(e1[PAD:PAD + n], host_ema(e0[PAD:PAD + n], w0[PAD:PAD + n], omd))
    assert same(e1[:PAD], e0[:PAD]) and same(e1[PAD + n:], e0[PAD + n:]), "written outside ema[0, n)"
    assert same(s.big_w, w0), "w was written"


def test_three_calls_follow_the_recurrence():
    n = 16384 + 7
    s = Slices(n, 7)
    e = s.e.cpu().numpy().copy()
    rng = np.random.RandomState(8)
    for k, omd in enumerate((f32(1) - f32(2.0) / f32(11.0), f32(1) - f32(3.0) / f32(12.0), f32(1) - f32(0.9))):
        w = rng.randn(n).astype(f32)
        s.w.copy_(torch.from_numpy(w))
        s.run(omd)
        e = host_ema(e, w, omd)
        assert same(s.e, e), "call %d" % k


def test_a_skipped_steps_record_leaves_the_averages_alone():
    """the record is built here and uploaded: {sumsq, norm, scale, flags, steps, clipped_steps, skipped_steps, pad}"""
    n = 2 * SHARE + 3
    s = Slices(n, 9)
    e0, w0 = s.big_e.cpu().numpy().copy(), s.big_w.cpu().numpy().copy()
    rec = np.zeros(8, np.uint32)
    rec[0:3] = np.array([np.inf, np.inf, 0.0], f32).view(np.uint32)
    rec[3], rec[4], rec[6] = _lib.CLIP_NONFINITE, 1, 1
    s.run(0.25, torch.from_numpy(rec.view(np.int32)).to(DEV))
    assert same(s.big_e, e0) and same(s.big_w, w0)
    rec[0:3] = np.array([4.0, 2.0, 0.5], f32).view(np.uint32)
    rec[3], rec[5], rec[6] = _lib.CLIP_CLIPPED, 1, 0             # the bit clear (a clipped step is a step): as NULL
    s.run(0.25, torch.from_numpy(rec.view(np.int32)).to(DEV))
    assert same(s.e, host_ema(e0[PAD:PAD + n], w0[PAD:PAD + n], 0.25))
    assert same(s.big_e[:PAD], e0[:PAD]) and same(s.big_e[PAD + n:], e0[PAD + n:]) and same(s.big_w, w0)


# ------------------------------------------------------------------------------------------- 2. the network
P, B = 20, 2


def _batches(net, k, seed):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    return [(torch.rand((B, net.S, net.S, 3), generator=gen), (torch.rand((B, P, P), generator=gen) < 0.3).to(torch.int64)) for _ in range(k)]


def _train(m, x, y, before_apply=None):
    m.x.copy_(x); m.labels.copy_(y)
    m.forward_device()
    m.backward_device(1.0 / (B * P * P))
    if before_apply is not None:
        before_apply(m)
    m.apply_adam(0.01) if m.optimizer == "adam" else m.apply_momentum(0.01, 0.9)
    torch.cuda.synchronize()


def _slots_equal(a, b):
    assert same(a.flat_w, b.flat_w) and same(a.flat_acc, b.flat_acc)
    if a.flat_v is not None:
        assert same(a.flat_v, b.flat_v)
    assert set(a.pk) == set(b.pk)
    for k in a.pk:
        assert torch.equal(a.pk[k].view(torch.int16), b.pk[k].view(torch.int16)), k


@pytest.mark.parametrize("optimizer", ["momentum", "adam"])
@pytest.mark.parametrize("L,dilated", [(2, False), (3, True)])
def test_averaging_net_beside_a_twin(L, dilated, optimizer):
    """training is not perturbed (weights, slots and packed copies of the two nets agree bit for bit after every step) and
    flat_ema[0:n_live) follows the host recurrence over the recorded weights at ema_decay_at(0.9, t); the dead dilated pair behind
    n_live (the (3, True) geometry has one) keeps the initial weights"""
    net = UNet(L, 16, dilated, B, P, seed=31, optimizer=optimizer, ema_decay=0.9)
    twin = UNet(L, 16, dilated, B, P, seed=31, optimizer=optimizer)
    assert twin.flat_ema is None and twin.ema == {} and twin.ema_decay is None
    assert net.flat_ema.dtype == torch.float32 and net.flat_ema.numel() == net.n_flat and set(net.ema) == set(net.names)
    assert (net.n_flat > net.n_live) == dilated
    w_init = net.flat_w.cpu().numpy().copy()
    assert same(net.flat_ema, w_init) and same(twin.flat_w, w_init)
    e, n = w_init.copy(), net.n_live
    for t, (x, y) in enumerate(_batches(net, 3, 3), start=1):
        _train(net, x, y)
        _train(twin, x, y)
        _slots_equal(net, twin)
        assert net.global_step == twin.global_step == t
        w = net.flat_w.cpu().numpy()
        assert not same(w[:n], e[:n])
        e[:n] = host_ema(e[:n], w[:n], f32(1) - ema_decay_at(0.9, t, True))
        assert same(net.flat_ema, e), "step %d" % t
        assert same(net.flat_ema[n:], w_init[n:])
    for name, (off, cnt, shape) in net._slices.items():   # the per-variable views look into flat_ema where the weights' views look into flat_w
        assert net.ema[name].data_ptr() == net.flat_ema.data_ptr() + 4 * off and tuple(net.ema[name].shape) == tuple(shape)


@pytest.mark.parametrize("optimizer", ["momentum", "adam"])
def test_a_step_with_an_inf_in_the_gradient_moves_no_average(optimizer):
    """clip_grad_norm=1e30 only measures and guards; step 2's gradient gets an inf: weights, slots, packed copies AND averages stay, the
    step still counts (the next step's decay is that of t = 3)"""
    net = UNet(2, 16, False, B, P, seed=33, optimizer=optimizer, clip_grad_norm=1e30, ema_decay=0.9)
    twin = UNet(2, 16, False, B, P, seed=33, optimizer=optimizer, clip_grad_norm=1e30)
    e, n = net.flat_w.cpu().numpy().copy(), net.n_live

    def poison(m):
        m.g["conv_1/conv1/kernel"].view(-1)[7] = float("inf")
    for t, (x, y) in enumerate(_batches(net, 3, 4), start=1):
        w_before = net.flat_w.clone()
        _train(net, x, y, poison if t == 2 else None)
        _train(twin, x, y, poison if t == 2 else None)
        _slots_equal(net, twin)
        if t == 2:
            assert same(net.flat_w, w_before) and net.clip_stats()["last_skipped"]
        else:
            e[:n] = host_ema(e[:n], net.flat_w.cpu().numpy()[:n], f32(1) - ema_decay_at(0.9, t, True))
        assert same(net.flat_ema, e), "step %d" % t
    assert net.clip_stats()["skipped"] == 1 and net.global_step == 3


def test_constructor_arguments():
    for bad in (1.0, 1, -0.1, float("nan"), float("inf"), "x", True, 0.999999999):
        with pytest.raises(RsuError):
            UNet(2, 16, False, B, P, ema_decay=bad)
    with pytest.raises(RsuError):
        UNet(2, 16, False, B, P, training=False, ema_decay=0.9)
    for off in (None, 0, 0.0):
        m = UNet(2, 16, False, B, P, ema_decay=off)
        assert m.ema_decay is None and m.flat_ema is None
    # without averages the context is a no-op: steps are allowed inside and nothing is exchanged
    x, y = _batches(m, 1, 5)[0]
    w0 = m.flat_w.clone()
    with m.averaged_weights():
        assert same(m.flat_w, w0)
        _train(m, x, y)
    assert m.global_step == 1 and not same(m.flat_w, w0)


def test_warmup_off_uses_the_decay_from_the_first_step():
    net = UNet(2, 16, False, B, P, seed=35, ema_decay=0.5, ema_warmup=False)
    e = net.flat_w.cpu().numpy().copy()
    x, y = _batches(net, 1, 6)[0]
    _train(net, x, y)
    assert same(net.flat_ema, host_ema(e, net.flat_w.cpu().numpy(), f32(0.5)))


# ------------------------------------------------------------------------------------------- 3. averaged_weights()
@pytest.fixture(scope="module")
def trained():
    """an averaging net and its twin, three steps in (built once; the tests below leave them in step with each other)"""
    net = UNet(3, 16, True, B, P, seed=37, ema_decay=0.9)
    twin = UNet(3, 16, True, B, P, seed=37)
    for x, y in _batches(net, 3, 7):
        _train(net, x, y)
        _train(twin, x, y)
    return net, twin


def _snapshot(m):
    return {"w": m.flat_w.clone(), "ema": m.flat_ema.clone(), "acc": m.flat_acc.clone(), "g": m.flat_g.clone(),
            "pk": {k: t.clone() for k, t in m.pk.items()}}


def _assert_snapshot(m, s):
    assert same(m.flat_w, s["w"]) and same(m.flat_ema, s["ema"]) and same(m.flat_acc, s["acc"]) and same(m.flat_g, s["g"])
    for k in s["pk"]:
        assert torch.equal(m.pk[k].view(torch.int16), s["pk"][k].view(torch.int16)), k


def test_forward_inside_the_block_reads_the_averages(trained):
    net, twin = trained
    before = _snapshot(net)
    assert not same(net.flat_w, net.flat_ema)
    fresh = UNet(3, 16, True, B, P, training=False, params={n: net.ema[n].cpu().numpy() for n in net.names})
    x = _batches(net, 1, 8)[0][0]
    fresh.x.copy_(x)
    fresh.forward_device(keep=1.0)
    net.x.copy_(x)
    net.forward_device(want_logits=True, keep=1.0)
    torch.cuda.synchronize()
    raw = net.prob.clone()
    with net.averaged_weights() as inside:
        assert inside is net
        assert same(net.flat_w, before["ema"]) and same(net.flat_ema, before["w"])
        net.forward_device(want_logits=True, keep=1.0)
        torch.cuda.synchronize()
        assert same(net.prob, fresh.prob)
        assert not same(net.prob, raw)
        for name, fn in (("apply_momentum", lambda: net.apply_momentum(0.01, 0.9)), ("backward_device", lambda: net.backward_device(1.0 / (B * P * P))),
                         ("averaged_weights", lambda: net.averaged_weights().__enter__()), ("state_dict", net.state_dict)):
            with pytest.raises(RsuError, match=name):
                fn()
    torch.cuda.synchronize()
    _assert_snapshot(net, before)
    net.forward_device(want_logits=True, keep=1.0)
    torch.cuda.synchronize()
    assert same(net.prob, raw)
    # an exception inside still exchanges back
    with pytest.raises(ZeroDivisionError):
        with net.averaged_weights():
            1 / 0
    torch.cuda.synchronize()
    _assert_snapshot(net, before)
    # one more training step equals the twin's
    x, y = _batches(net, 1, 9)[0]
    _train(net, x, y)
    _train(twin, x, y)
    _slots_equal(net, twin)
    assert same(net.flat_g, twin.flat_g)


# ------------------------------------------------------------------------------------------- 4. checkpoints
def test_state_dict_round_trip(trained):
    net, _ = trained
    d = net.state_dict()
    assert {k for k in d if "Exponential" in k} == {n + "/ExponentialMovingAverage" for n in net.names} and EMA_SUFFIX == "/ExponentialMovingAverage"
    for n in net.names:
        assert d[n + EMA_SUFFIX].shape == d[n].shape and same(d[n + EMA_SUFFIX], net.ema[n])
    a = UNet(3, 16, True, B, P, seed=1, ema_decay=0.9)
    a.load_state_dict(d)
    assert same(a.flat_ema, net.flat_ema) and same(a.flat_w, net.flat_w) and same(a.flat_acc, net.flat_acc) and a.global_step == net.global_step
    b = UNet(3, 16, True, B, P, seed=1)
    b.load_state_dict(d)                      # a net without averaging ignores the keys
    assert b.flat_ema is None and same(b.flat_w, net.flat_w) and not any("Exponential" in k for k in b.state_dict())
    c = UNet(3, 16, True, B, P, seed=1, ema_decay=0.9)
    c.load_state_dict(b.state_dict())         # a checkpoint without the keys: the averages become the loaded weights
    assert same(c.flat_w, net.flat_w)
    for n in c.names:
        assert same(c.ema[n], net.w[n])
    # resuming continues both exactly
    x, y = _batches(net, 1, 10)[0]
    twin = trained[1]
    _train(net, x, y)
    _train(twin, x, y)
    _train(a, x, y)
    assert same(a.flat_w, net.flat_w) and same(a.flat_ema, net.flat_ema)


def test_restore_from_tf_arrays_maps_the_shadow_names(trained):
    from road_segmentation_unet_amd.model import ConvolutionalModel, Options
    net, _ = trained
    arrays = {"scope/" + k + ":0": v for k, v in net.state_dict().items()}
    m = ConvolutionalModel(Options(num_layers=3, root_size=16, patch_size=P, batch_size=B, dilated_layers=True, logdir=None, ema_decay=0.9), device=DEV)
    m.restore_from_tf_arrays(arrays)
    assert same(m.net.flat_ema, net.flat_ema) and same(m.net.flat_w, net.flat_w)


# ------------------------------------------------------------------------------------------- 5. the driver
def _model(**kw):
    from road_segmentation_unet_amd.model import ConvolutionalModel, Options
    o = dict(num_layers=2, root_size=16, patch_size=P, batch_size=B, dropout=1.0, lr=0.05, seed=5, logdir=None)
    o.update(kw)
    return ConvolutionalModel(Options(**o), device=DEV)


def test_model_evaluates_and_predicts_with_the_averages():
    m = _model(ema_decay=0.5)
    S = m.input_size
    rng = np.random.RandomState(11)
    for _ in range(4):
        m.train_step(rng.rand(B, S, S, 3).astype(f32), (rng.rand(B, P, P) < 0.3).astype(np.int64))
    X, y = rng.rand(3, S, S, 3).astype(f32), (rng.rand(3, P, P) < 0.3).astype(np.int64)
    before = _snapshot(m.net)
    avg, raw, default = m.evaluate(X, y, averaged=True), m.evaluate(X, y, averaged=False), m.evaluate(X, y)
    torch.cuda.synchronize()
    _assert_snapshot(m.net, before)               # "training is left as it was" covers the exchange
    assert avg["averaged"] is True and raw["averaged"] is False and default["averaged"] is True
    assert not np.array_equal(avg["sums"], raw["sums"])
    assert np.array_equal(avg["sums"], default["sums"]) and np.array_equal(avg["hist"], default["hist"])
    imgs = rng.rand(1, 36, 36, 3).astype(f32)     # (36 - 20) % 16 == 0: a 2 x 2 window of tiles, through the window nets
    p_avg, p_raw, p_default = m.predict(imgs, averaged=True), m.predict(imgs, averaged=False), m.predict(imgs)
    assert same(p_avg, p_default) and not same(p_avg, p_raw)
    _assert_snapshot(m.net, before)
    # a model whose RAW weights are the averages scores and predicts the same bits
    plain = _model()
    sd = m.net.state_dict()
    plain.net.load_state_dict({n: sd[n + EMA_SUFFIX] for n in m.net.names})
    ref = plain.evaluate(X, y)
    assert ref["averaged"] is False
    assert np.array_equal(ref["sums"], avg["sums"]) and np.array_equal(ref["hist"], avg["hist"]) and ref["f1"] == avg["f1"]
    assert same(plain.predict(imgs), p_avg)
    with pytest.raises(ValueError, match="averaged"):
        plain.evaluate(X, y, averaged=True)
    with pytest.raises(ValueError, match="averaged"):
        plain.predict(imgs, averaged=True)


def test_cli_trains_validates_and_saves_with_the_averages(tmp_path, capsys):
    from PIL import Image
    from road_segmentation_unet_amd.cli import main
    rng = np.random.RandomState(4)
    tr = tmp_path / "train"
    (tr / "images").mkdir(parents=True)
    (tr / "groundtruth").mkdir(parents=True)
    H = 48
    for i in range(4):
        img = (rng.rand(H, H, 3) * 255).astype(np.uint8)
        gt = ((img[..., 0] > 127) * 255).astype(np.uint8)
        Image.fromarray(img).save(tr / "images" / ("satImage_%03d.png" % i))
        Image.fromarray(gt).save(tr / "groundtruth" / ("satImage_%03d.png" % i))
    runs = tmp_path / "runs"
    argv = ["--num_layers=2", "--root_size=16", "--patch_size=16", "--stride=16", "--batch_size=4", "--num_epoch=1", "--lr=0.001",
            "--ema_decay=0.9", "--validation_images=1", "--save_best", "--train_data_dir=%s" % tr, "--save_path=%s" % runs,
            "--logdir=%s" % (tmp_path / "logs"), "--rotation_angles=0,90", "--seed=5"]
    assert main(argv) == 0
    out = capsys.readouterr().out
    line = [ln for ln in out.splitlines() if re.search(r"step \d+ validation:", ln)]
    assert line and all(ln.endswith("(averaged weights)") for ln in line), out[-2000:]
    files = sorted(str(p.relative_to(runs)) for p in runs.rglob("*.npz"))
    assert len(files) == 2 and any(f.endswith("-best.chkpt.npz") for f in files) and any(f.endswith("model-epoch-000.chkpt.npz") for f in files)
    for f in files:
        with np.load(os.path.join(str(runs), f)) as z:
            keys = [k.replace("|", "/") for k in z.files]
            shadows = [k for k in keys if k.endswith(EMA_SUFFIX)]
            assert len(shadows) == len(param_shapes(2, 16, False)) and all(k[:-len(EMA_SUFFIX)] in keys for k in shadows), f
            assert not np.array_equal(z["conv_0|conv1|kernel"], z["conv_0|conv1|kernel|ExponentialMovingAverage"])
