"""-m gpu: weight decay and the learning-rate schedules through the network, the model and the command line. A decaying net runs beside
a twin WITHOUT decay whose state is transformed by separate torch ops in front of its plain update pass -- decoupled: the packed-kernel
ranges of flat_w pre-decayed (mul, then sub); l2 under Adam: flat_g turned into f32(f32(gscale g) + f32(lambda w)) and stepped with
gscale 1 -- and must end with the same BITS in flat_w, the slots and the packed copies. l2 under Momentum is held to the tolerance
tests/test_gpu_fenced.py grants the Momentum rule (its mu * acc + gscale * g may be contracted, so two kernels' bits cannot be promised
equal). tests/test_gpu_optim_fenced.py holds the two entries themselves to the existing ones inside fenced arenas."""
import json
import os
import re

import numpy as np
import pytest
import torch

from road_segmentation_unet_amd import optim as optim_mod
from road_segmentation_unet_amd import unet as unet_mod
from road_segmentation_unet_amd._lib import RsuError
from road_segmentation_unet_amd.unet import UNet, ema_decay_at, lr_at
from tests.accum_util import same

pytestmark = pytest.mark.gpu

f32 = np.float32
P, B = 20, 2
LR, LAMBDA = 0.01, 0.1          # lr * lambda = 1e-3: a step's decay is far above every tolerance here
RTOL, ATOL = 1e-6, 1e-7         # tests/test_gpu_fenced.py test_update_and_pack_tables, the Momentum rule
INV = 1.0 / (B * P * P)


def _net(optimizer, **kw):
    return UNet(2, 16, False, B, P, seed=71, optimizer=optimizer, **kw)


def _batches(net, k, seed):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    return [(torch.rand((B, net.S, net.S, 3), generator=gen), (torch.rand((B, P, P), generator=gen) < 0.3).to(torch.int64)) for _ in range(k)]


def _passes(m, x, y):
    m.x.copy_(x); m.labels.copy_(y)
    m.forward_device()
    m.backward_device(INV)


def _apply(m, gscale=1.0):
    m.apply_adam(LR, gscale=gscale) if m.optimizer == "adam" else m.apply_momentum(LR, 0.9, gscale=gscale)
    torch.cuda.synchronize()


def _kernel_ranges(m):
    """(offset, count) in the flat buffers of every variable that decays: the packed kernels of the update table"""
    return [m._slices[n][:2] for _kind, n, _sh, _segs in m._packed_kernels()]


def _slots_equal(a, b):
    assert same(a.flat_w, b.flat_w) and same(a.flat_acc, b.flat_acc)
    if a.flat_v is not None:
        assert same(a.flat_v, b.flat_v)
    for k in a.pk:
        assert torch.equal(a.pk[k].view(torch.int16), b.pk[k].view(torch.int16)), k


def _packs_are_packs_of_the_weights(m):
    got = {k: t.clone() for k, t in m.pk.items()}
    m.repack()
    torch.cuda.synchronize()
    for k in got:
        assert torch.equal(got[k].view(torch.int16), m.pk[k].view(torch.int16)), k


@pytest.mark.parametrize("clip", [None, 0.01], ids=["noclip", "clip"])
@pytest.mark.parametrize("optimizer", ["momentum", "adam"])
def test_decoupled_decay_beside_a_pre_decayed_twin(optimizer, clip):
    net = _net(optimizer, weight_decay=LAMBDA, clip_grad_norm=clip)
    twin = _net(optimizer, clip_grad_norm=clip)
    assert net.weight_decay == LAMBDA and net.weight_decay_mode == "decoupled" and twin.weight_decay is None
    assert set(net.state_dict()) == set(twin.state_dict())          # decay adds no state
    ranges = _kernel_ranges(twin)
    decays, live = net.decaying_parameters()
    assert decays == sum(c for _, c in ranges) and 0 < decays < live <= net.n_live
    for step, (x, y) in enumerate(_batches(net, 3, 72)):
        _passes(net, x, y)
        twin.flat_g.copy_(net.flat_g)
        w0 = twin.flat_w.clone()
        d = float(f32(lr_at(step, LR)) * f32(LAMBDA))
        for o, c in ranges:                                           # two separate float32 roundings: d * w, then w - (d * w)
            w = twin.flat_w[o:o + c]
            w.sub_(w.mul(d))
        assert not same(twin.flat_w, w0)
        _apply(net)
        _apply(twin)
        _slots_equal(net, twin)
        assert net.global_step == twin.global_step == step + 1
    if clip is not None:
        st = net.clip_stats()
        assert st["steps"] == 3 and st["clipped"] >= 1 and st["skipped"] == 0 and st == twin.clip_stats()
    _packs_are_packs_of_the_weights(net)


def test_adam_l2_beside_a_twin_with_the_transformed_gradient():
    net = _net("adam", weight_decay=LAMBDA, weight_decay_mode="l2")
    twin = _net("adam")
    ranges, gs, lam = _kernel_ranges(twin), 0.5, float(f32(LAMBDA))
    for step, (x, y) in enumerate(_batches(net, 3, 73)):
        _passes(net, x, y)
        g = net.flat_g.mul(gs)                                        # f32(gscale g), everywhere
        for o, c in ranges:
            g[o:o + c].add_(twin.flat_w[o:o + c].mul(lam))           # + f32(lambda w) on what decays: one more rounding
        twin.flat_g.copy_(g)
        _apply(net, gscale=gs)
        _apply(twin, gscale=1.0)
        _slots_equal(net, twin)
    _packs_are_packs_of_the_weights(net)


def test_momentum_l2_one_step_against_the_twin():
    net = _net("momentum", weight_decay=LAMBDA, weight_decay_mode="l2")
    twin, plain = _net("momentum"), _net("momentum")
    ranges, gs, lam = _kernel_ranges(twin), 0.5, float(f32(LAMBDA))
    x, y = _batches(net, 1, 74)[0]
    _passes(net, x, y)
    net.flat_acc.copy_(net.flat_g * 0.3)                              # (slots that are not zero: mu * acc takes part)
    twin.flat_acc.copy_(net.flat_acc); plain.flat_acc.copy_(net.flat_acc)
    plain.flat_g.copy_(net.flat_g)
    g = net.flat_g.mul(gs)
    for o, c in ranges:
        g[o:o + c].add_(twin.flat_w[o:o + c].mul(lam))
    twin.flat_g.copy_(g)
    _apply(net, gscale=gs)
    _apply(twin, gscale=1.0)
    _apply(plain, gscale=gs)
    n = net.n_live
    for a, b in ((net.flat_w, twin.flat_w), (net.flat_acc, twin.flat_acc)):
        np.testing.assert_allclose(a.cpu().numpy()[:n], b.cpu().numpy()[:n], rtol=RTOL, atol=ATOL)
    _packs_are_packs_of_the_weights(net)
    # the decay is there (about lr * lambda * |w| on the kernels), and only there
    wn, wp = net.flat_w.cpu().numpy().astype(np.float64), plain.flat_w.cpu().numpy().astype(np.float64)
    mask = np.zeros(net.n_flat, bool)
    for o, c in ranges:
        mask[o:o + c] = True
    far = np.abs(wn - wp)[mask] > 100.0 * (ATOL + RTOL * np.abs(wp[mask]))
    assert far.mean() > 0.5, float(far.mean())
    assert same(net.flat_w.cpu().numpy()[~mask], plain.flat_w.cpu().numpy()[~mask])


@pytest.mark.parametrize("mode", ["decoupled", "l2"])
@pytest.mark.parametrize("optimizer", ["momentum", "adam"])
def test_a_skipped_step_decays_nothing(optimizer, mode):
    net = _net(optimizer, weight_decay=LAMBDA, weight_decay_mode=mode, clip_grad_norm=1e30)
    x, y = _batches(net, 1, 75)[0]
    _passes(net, x, y)
    net.g["conv_1/conv1/kernel"].view(-1)[7] = float("inf")
    w0, a0 = net.flat_w.clone(), net.flat_acc.clone()
    v0 = net.flat_v.clone() if net.flat_v is not None else None
    pk0 = {k: t.clone() for k, t in net.pk.items()}
    _apply(net)
    st = net.clip_stats()
    assert st["skipped"] == 1 and st["last_skipped"] and net.global_step == 1
    assert same(net.flat_w, w0) and same(net.flat_acc, a0) and (v0 is None or same(net.flat_v, v0))
    for k in pk0:
        assert torch.equal(net.pk[k].view(torch.int16), pk0[k].view(torch.int16)), k
    _passes(net, x, y)                                                # the next, finite step moves and decays
    _apply(net)
    assert net.clip_stats()["skipped"] == 1 and not same(net.flat_w, w0)


def test_the_moving_average_follows_the_decayed_weights():
    from tests.test_gpu_ema import host_ema
    net, plain = _net("adam", weight_decay=LAMBDA, ema_decay=0.9), _net("adam", ema_decay=0.9)
    e, n = net.flat_w.cpu().numpy().copy(), net.n_live
    for t, (x, y) in enumerate(_batches(net, 2, 76), 1):
        for m in (net, plain):
            _passes(m, x, y)
            _apply(m)
        e[:n] = host_ema(e[:n], net.flat_w.cpu().numpy()[:n], f32(1) - ema_decay_at(0.9, t, True))
        assert same(net.flat_ema, e), "step %d" % t
    assert not same(net.flat_w, plain.flat_w) and not same(net.flat_ema, plain.flat_ema)


@pytest.mark.parametrize("optimizer", ["momentum", "adam"])
def test_without_decay_the_net_issues_the_calls_it_always_did(optimizer, monkeypatch):
    names = {}
    real = unet_mod.call
    who = [None]
    for mod in (unet_mod, optim_mod):   # (the passes' calls and the optimizer step's)
        monkeypatch.setattr(mod, "call", lambda name, *a: (names.setdefault(who[0], []).append(name), real(name, *a))[1])
    nets = {"none": _net(optimizer, weight_decay=None), "plain": _net(optimizer), "decay": _net(optimizer, weight_decay=LAMBDA)}
    for x, y in _batches(nets["plain"], 2, 77):
        for who[0], m in nets.items():
            _passes(m, x, y)
            _apply(m)
    assert names["none"] == names["plain"] and not [n for n in names["plain"] if "decay" in n]
    _slots_equal(nets["none"], nets["plain"])
    run = "rsu_update_table_run_adam" if optimizer == "adam" else "rsu_update_table_run"
    assert names["plain"].count(run) == 2 and names["decay"].count(run + "_decay") == 2 and run not in names["decay"]
    assert [n for n in names["decay"] if n != run + "_decay"] == [n for n in names["plain"] if n != run]   # one launch for one launch
    assert not same(nets["decay"].flat_w, nets["plain"].flat_w)


def test_constructor_and_environment(monkeypatch):
    for bad in (0, 0.0, -1e-4, float("nan"), float("inf"), "x", True):
        with pytest.raises(ValueError):
            _net("momentum", weight_decay=bad)
    for bad in ("adamw", "L2", None, 1):
        with pytest.raises(ValueError):
            _net("adam", weight_decay=LAMBDA, weight_decay_mode=bad)
    with pytest.raises(ValueError):
        UNet(2, 16, False, B, P, training=False, weight_decay=LAMBDA)
    assert UNet(2, 16, False, B, P, training=False).weight_decay is None
    for optimizer in ("momentum", "adam"):
        net = _net(optimizer, weight_decay=LAMBDA)
        x, y = _batches(net, 1, 78)[0]
        _passes(net, x, y)
        w0 = net.flat_w.clone()
        monkeypatch.setenv("RSU_FUSED_UPDATE", "0")
        with pytest.raises(RsuError, match="RSU_FUSED_UPDATE"):
            _apply(net)
        monkeypatch.delenv("RSU_FUSED_UPDATE")
        torch.cuda.synchronize()
        assert net.global_step == 0 and same(net.flat_w, w0) and getattr(net, "beta1_power", None) is None
        with pytest.raises(ValueError):
            net.set_lr_schedule("cosine")                             # no horizon
        _apply(net)
        assert net.global_step == 1 and not same(net.flat_w, w0)


def test_the_net_steps_at_the_scheduled_rate(monkeypatch):
    """learning_rate() is lr_at at the net's step, and that float is the rate the update pass receives"""
    net = _net("momentum", weight_decay=LAMBDA)
    net.set_lr_schedule("cosine", 2, 10, 0.1)
    seen = []
    real = unet_mod.call
    for mod in (unet_mod, optim_mod):   # (the passes' calls and the optimizer step's)
        monkeypatch.setattr(mod, "call", lambda name, *a: (seen.append((name, a)), real(name, *a))[1])
    x, y = _batches(net, 1, 79)[0]
    for t in range(4):
        want = lr_at(t, LR, "cosine", 2, 10, 0.1)
        assert net.learning_rate(LR) == want
        _passes(net, x, y)
        _apply(net)
        name, a = [s for s in seen if s[0] == "rsu_update_table_run_decay"][-1]
        assert a[3] == want and a[6] == float(f32(want) * f32(LAMBDA)) and a[7] == 1, (t, a[3:8])
    assert lr_at(0, LR, "cosine", 2, 10, 0.1) == float(f32(LR * 0.5)) and lr_at(1, LR, "cosine", 2, 10, 0.1) < LR


def test_cli_trains_with_decay_and_a_cosine_schedule(tmp_path, capsys):
    from PIL import Image
    from road_segmentation_unet_amd.cli import main
    rng = np.random.RandomState(4)
    tr = tmp_path / "train"
    (tr / "images").mkdir(parents=True)
    (tr / "groundtruth").mkdir(parents=True)
    H = 48
    for i in range(2):
        img = (rng.rand(H, H, 3) * 255).astype(np.uint8)
        gt = ((img[..., 0] > 127) * 255).astype(np.uint8)
        Image.fromarray(img).save(tr / "images" / ("satImage_%03d.png" % i))
        Image.fromarray(gt).save(tr / "groundtruth" / ("satImage_%03d.png" % i))
    logs, runs = tmp_path / "logs", tmp_path / "runs"
    argv = ["--num_layers=2", "--root_size=16", "--patch_size=16", "--stride=16", "--batch_size=4", "--num_epoch=1", "--lr=0.001",
            "--optimizer=adam", "--weight_decay=1e-4", "--lr_schedule=cosine", "--lr_warmup_steps=2", "--train_data_dir=%s" % tr,
            "--save_path=%s" % runs, "--logdir=%s" % logs, "--rotation_angles=0,90", "--seed=5"]
    assert main(argv) == 0
    out = capsys.readouterr().out
    steps = len(range(0, 36 - 4, 4))                                  # 2 images x 2 angles x 9 patches, the last batch dropped
    assert re.search(r"Weight decay: decoupled lambda 0\.0001, (\d+) of (\d+) live parameters decay", out), out[-2000:]
    m = re.search(r"Learning-rate schedule: cosine over (\d+) optimizer steps", out)
    assert m and int(m.group(1)) == steps == 8, out[-2000:]
    files = sorted(runs.rglob("model-epoch-000.chkpt.npz"))
    assert len(files) == 1
    with np.load(str(files[0])) as z:
        assert int(z["global_step"]) == steps and np.isfinite(z["conv_0|conv1|kernel"]).all()
        assert not [k for k in z.files if "decay" in k.lower()]       # no new state
    run_dirs = os.listdir(logs)
    assert len(run_dirs) == 1
    events = [json.loads(line) for line in open(logs / run_dirs[0] / "events.jsonl")]
    rates = [e for e in events if e["tag"] == "learning_rate"]
    assert [e["step"] for e in rates] == list(range(1, steps + 1))
    for e in rates:                                                   # (logged behind the step: the rate of the step that follows)
        assert e["value"] == lr_at(e["step"], 0.001, "cosine", 2, steps, 0.0), e
    values = [e["value"] for e in rates]                              # (the two warm-up steps are t = 0 and 1: the first logged rate is past them)
    assert all(b < a for a, b in zip(values, values[1:])) and values[0] < 0.001 and values[-1] == 0.0
