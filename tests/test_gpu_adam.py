"""-m gpu: tf.train.AdamOptimizer on the HIP path -- the plain kernel (rsu_adam_step) and the Adam instantiation of the one-launch
update + re-pack pass (rsu_update_table_run_adam) against a numpy float32 restatement of TensorFlow 1.x ApplyAdam, the network's
trajectory, checkpoints under TensorFlow's names, data parallelism, the command line and a short training run."""
import os
import re
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from road_segmentation_unet_amd._lib import RsuError, call

pytestmark = pytest.mark.gpu

f32 = np.float32


def power(beta, t):
    """beta^t as AdamOptimizer's float32 accumulator holds it: beta, multiplied by beta after every step"""
    p = f32(beta)
    for _ in range(t - 1):
        p = f32(p * f32(beta))
    return p


def np_adam(w, m, v, g, alpha, beta1, beta2, epsilon, gscale=1.0):
    """ApplyAdam (TensorFlow 1.x, float32, its operation order); returns new (w, m, v)"""
    gs = f32(gscale) * g.astype(f32)
    m = m + (gs - m) * (f32(1) - f32(beta1))
    v = v + (gs * gs - v) * (f32(1) - f32(beta2))
    w = w - (m * f32(alpha)) / (np.sqrt(v) + f32(epsilon))
    return w, m, v


def tf_alpha(lr0, global_step, beta1_power, beta2_power):
    """AdamOptimizer's step size at exponential_decay(lr0, global_step, 1000, 0.95, staircase=True), float32"""
    lr_t = f32(lr0) * f32(0.95) ** f32(global_step // 1000)
    return lr_t * np.sqrt(f32(1) - f32(beta2_power)) / (f32(1) - f32(beta1_power))


def assert_close_ulp(got, ref, what, rtol=1e-6, ulps=4):
    """rtol 1e-6, plus an atol of a few ulp of the tensor's largest element for entries near zero"""
    atol = ulps * float(np.spacing(f32(np.abs(ref).max()))) if ref.size else 0.0
    np.testing.assert_allclose(got, ref, rtol=rtol, atol=atol, err_msg=what)


# ------------------------------------------------------------------------------------------- the op
@pytest.mark.parametrize("gscale", [1.0, 0.5])
def test_adam_step_op(gscale):
    rng = np.random.RandomState(31)
    n = 1003   # odd tail: the scalar path of the kernel
    w = rng.randn(n).astype(f32)
    m = (rng.randn(n) * 1e-2).astype(f32)
    v = (rng.rand(n) * 1e-4).astype(f32)
    g = (rng.randn(n) * 1e-2).astype(f32)
    g[:7] = 0.0
    v[:3] = 0.0    # sqrt(0) + epsilon
    alpha, b1, b2, eps = 1.234e-3, 0.9, 0.999, 1e-8
    dev = [torch.full((n + 1,), 7.0, device="cuda:0") for _ in range(4)]   # element n: padding that must stay untouched
    for t, a in zip(dev, (w, m, v, g)):
        t[:n] = torch.from_numpy(a).cuda()
    wd, md, vd, gd = dev
    call("rsu_adam_step", wd.data_ptr(), md.data_ptr(), vd.data_ptr(), gd.data_ptr(), alpha, b1, b2, eps, gscale, n,
         torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    rw, rm, rv = np_adam(w, m, v, g, f32(alpha), b1, b2, eps, gscale)
    for t, r, name in ((wd, rw, "w"), (md, rm, "m"), (vd, rv, "v")):
        got = t.cpu().numpy()
        np.testing.assert_allclose(got[:n], r, rtol=1e-6, atol=0, err_msg=name)
        assert got[n] == 7.0, name
    assert gd.cpu().numpy()[n] == 7.0


def test_adam_step_op_rejects_misaligned_pointers():
    from road_segmentation_unet_amd._lib import lib
    t = torch.zeros(64, device="cuda:0")
    p, st = t.data_ptr(), torch.cuda.current_stream().cuda_stream
    assert lib().rsu_adam_step(p + 4, p, p, p, 1e-3, 0.9, 0.999, 1e-8, 1.0, 8, st) < 0
    assert lib().rsu_adam_step(None, p, p, p, 1e-3, 0.9, 0.999, 1e-8, 1.0, 8, st) < 0
    assert not torch.any(t)


# ------------------------------------------------------------------------------------------- the network
def _net(L, root, dilated, P, B, seed=17, optimizer="adam"):
    from road_segmentation_unet_amd.unet import UNet
    return UNet(L, root, dilated, B, P, seed=seed, training=True, optimizer=optimizer)


def _batch(m, gen):
    m.x.copy_(torch.rand((m.B, m.S, m.S, 3), generator=gen))
    m.labels.copy_((torch.rand((m.B, m.P, m.P), generator=gen) < 0.3).to(torch.int64))


@pytest.mark.parametrize("L,root,dilated,P", [(3, 16, True, 20), (2, 16, False, 20)])
def test_adam_table_equals_plain_step_then_repack(L, root, dilated, P, monkeypatch):
    """rsu_update_table_run_adam (Adam + both packed layouts from ONE read of w, m, v, g) against rsu_adam_step over [0, n_live) followed
    by the batched re-pack, on the same gradient: w, m, v and every packed buffer bit for bit. L=3 dilated has three concat sources, the
    transposed convs, the first conv and the dead pair; m and v start from non-zero values so every slot matters."""
    m = _net(L, root, dilated, P, 2)
    gen = torch.Generator(device="cpu").manual_seed(6)
    _batch(m, gen)
    m.forward_device()
    m.backward_device(1.0 / (2 * P * P))
    n = m.n_live
    m.flat_acc[:n].copy_(torch.randn(n, generator=gen) * 1e-3)
    m.flat_v[:n].copy_(torch.rand(n, generator=gen) * 1e-6)
    m.global_step = 5
    m.beta1_power, m.beta2_power = power(0.9, 6), power(0.999, 6)
    start = (m.flat_w.clone(), m.flat_acc.clone(), m.flat_v.clone(), m.global_step, m.beta1_power, m.beta2_power)
    out = {}
    for fused in ("1", "0"):
        monkeypatch.setenv("RSU_FUSED_UPDATE", fused)
        m.flat_w.copy_(start[0]); m.flat_acc.copy_(start[1]); m.flat_v.copy_(start[2])
        m.global_step, m.beta1_power, m.beta2_power = start[3:]
        m.repack()
        m.apply_adam(0.01, 0.9, 0.999, 1e-8)
        torch.cuda.synchronize()
        out[fused] = (m.flat_w.clone(), m.flat_acc.clone(), m.flat_v.clone(), {k: t.clone() for k, t in m.pk.items()},
                      (m.global_step, m.beta1_power, m.beta2_power))
    a, b = out["1"], out["0"]
    for i, what in enumerate(("w", "m", "v")):
        assert torch.equal(a[i], b[i]), what
    assert not torch.equal(a[0], start[0])
    for k in a[3]:
        assert torch.equal(a[3][k].view(torch.int16), b[3][k].view(torch.int16)), k
    assert a[4] == b[4] == (6, power(0.9, 7), power(0.999, 7))
    # the dead level-(L-1) dilated pair (behind n_live) is never stepped
    assert torch.equal(a[0][n:], start[0][n:]) and not torch.any(a[1][n:]) and not torch.any(a[2][n:])


def _trajectory(L=3, root=16, dilated=True, P=20, B=2, steps=3, lr0=0.01, check=True):
    m = _net(L, root, dilated, P, B, seed=23)
    m.global_step = 999   # the staircase decay engages after the first step
    gen = torch.Generator(device="cpu").manual_seed(8)
    n = m.n_live
    dead0 = m.flat_w[n:].clone()
    b1p, b2p = f32(0.9), f32(0.999)
    for t in range(steps):
        _batch(m, gen)
        m.forward_device()
        m.backward_device(1.0 / (B * P * P))
        torch.cuda.synchronize()
        w0, m0, v0, g = (x[:n].cpu().numpy() for x in (m.flat_w, m.flat_acc, m.flat_v, m.flat_g))
        gs = m.global_step
        m.apply_adam(lr0, 0.9, 0.999, 1e-8)
        torch.cuda.synchronize()
        if check:
            rw, rm, rv = np_adam(w0, m0, v0, g, tf_alpha(lr0, gs, b1p, b2p), 0.9, 0.999, 1e-8)
            assert_close_ulp(m.flat_acc[:n].cpu().numpy(), rm, "m step %d" % t)
            assert_close_ulp(m.flat_v[:n].cpu().numpy(), rv, "v step %d" % t)
            assert_close_ulp(m.flat_w[:n].cpu().numpy(), rw, "w step %d" % t)
        b1p, b2p = b1p * f32(0.9), b2p * f32(0.999)
        assert m.global_step == gs + 1 and m.beta1_power == b1p and m.beta2_power == b2p
    assert m.n_flat > n   # (L=3 dilated: the dead pair exists)
    assert torch.equal(m.flat_w[n:], dead0) and not torch.any(m.flat_acc[n:]) and not torch.any(m.flat_v[n:])
    return m


def test_adam_trajectory_matches_numpy_adam_of_its_own_gradients():
    """three forward / backward / apply_adam steps; each step against the numpy ApplyAdam of the HIP's own flat_g (not of oracle
    gradients: Adam's first step is about lr * sign(g), so tiny gradients would amplify bf16 noise; gradient parity is tested
    elsewhere). global_step starts at 999: the decayed rate changes between the first and the second step."""
    _trajectory()


def test_adam_runs_are_bit_identical():
    a, b = _trajectory(check=False), _trajectory(check=False)
    for x, y in ((a.flat_w, b.flat_w), (a.flat_acc, b.flat_acc), (a.flat_v, b.flat_v)):
        assert torch.equal(x, y)


def test_optimizers_refuse_each_others_steps():
    m = _net(2, 16, False, 20, 2)
    with pytest.raises(RsuError):
        m.apply_momentum(0.01, 0.9)
    m.forward_device()
    with pytest.raises(RsuError):
        m.backward_device(1.0 / 800, update=(0.01, 0.9))   # update= names a Momentum step
    mm = _net(2, 16, False, 20, 2, optimizer="momentum")
    assert mm.flat_v is None
    with pytest.raises(RsuError):
        mm.apply_adam(0.01)
    with pytest.raises(RsuError):
        _net(2, 16, False, 20, 2, optimizer="sgd")


# ------------------------------------------------------------------------------------------- checkpoints
LM, RM, PM, BM = 3, 16, 20, 2


def _model(**kw):
    from oracle import unet_oracle as U
    from road_segmentation_unet_amd.model import ConvolutionalModel, Options
    o = dict(num_layers=LM, root_size=RM, patch_size=PM, batch_size=BM, dilated_layers=True, dropout=1.0, lr=0.01, seed=3,
             optimizer="adam", adam_beta1=0.85, adam_beta2=0.995, adam_epsilon=1e-7)
    o.update(kw)
    return ConvolutionalModel(Options(**o), device="cuda:0", params=U.init_params(LM, RM, True, seed=13, bias_scale=0.05))


def _ckpt_data(steps):
    from road_segmentation_unet_amd.unet import input_size_needed
    rng = np.random.RandomState(41)
    S = input_size_needed(PM, LM)
    return [(rng.rand(BM, S, S, 3).astype(f32), (rng.rand(BM, PM, PM) < 0.3).astype(np.float64)) for _ in range(steps)]


def _state(model):
    torch.cuda.synchronize()
    return model.net.state_dict()


def test_adam_checkpoint_names_and_resume(tmp_path):
    data = _ckpt_data(3)
    a = _model()
    for X, y in data[:2]:
        a.train_step(X, y)
    sd = _state(a)
    names = a.net.names
    assert set(sd) == set(names) | {n + "/Adam" for n in names} | {n + "/Adam_1" for n in names} | {"beta1_power", "beta2_power", "global_step"}
    assert sd["beta1_power"].dtype == np.float32 and sd["beta1_power"] == power(0.85, 3)
    assert sd["beta2_power"] == power(0.995, 3) and int(sd["global_step"]) == 2
    path = a.save_as(str(tmp_path / "ck" / "model.chkpt"))
    a.train_step(*data[2])
    cont = _state(a)
    b = _model()
    b.restore(file=path)
    assert b.net.global_step == 2 and b.net.beta1_power == power(0.85, 3)
    b.train_step(*data[2])
    resumed = _state(b)
    for k in cont:
        np.testing.assert_array_equal(resumed[k], cont[k], err_msg=k)


def test_restore_from_tf_arrays_reads_adam_slots_and_powers():
    a = _model()
    for X, y in _ckpt_data(2):
        a.train_step(X, y)
    sd = _state(a)
    arrays = {"unet/" + k + ":0": v for k, v in sd.items()}   # the names of a scoped TensorFlow graph, with the tensor suffix
    b = _model()
    b.restore_from_tf_arrays(arrays)
    got = _state(b)
    assert set(got) == set(sd)
    for k in sd:
        np.testing.assert_array_equal(got[k], sd[k], err_msg=k)
    assert np.any(got["conv_0/conv1/kernel/Adam_1"])


def test_momentum_checkpoint_into_adam_model_resets_the_optimizer():
    data = _ckpt_data(2)
    mom = _model(optimizer="momentum")
    mom.train_step(*data[0])
    msd = _state(mom)
    assert np.any(msd["conv_0/conv1/kernel/Momentum"])
    b = _model()
    b.train_step(*data[1])   # (non-zero slots and powers that the load must reset)
    b.net.load_state_dict(msd)
    got = _state(b)
    assert not any(k.endswith("/Momentum") for k in got) and "beta1_power" not in got
    for n in b.net.names:
        np.testing.assert_array_equal(got[n], msd[n], err_msg=n)
        assert not np.any(got[n + "/Adam"]) and not np.any(got[n + "/Adam_1"]), n
    assert int(got["global_step"]) == 1
    b.train_step(*data[1])
    after = _state(b)
    assert after["beta1_power"] == power(0.85, 2) and after["beta2_power"] == power(0.995, 2)
    # and a Momentum model ignores Adam keys: the Adam model's checkpoint loads its weights and leaves the Momentum slots alone
    before = mom.net.flat_acc.clone()
    mom.net.load_state_dict(after)
    assert torch.equal(mom.net.flat_acc, before)
    np.testing.assert_array_equal(_state(mom)["conv_0/conv1/kernel"], after["conv_0/conv1/kernel"])


# ------------------------------------------------------------------------------------------- data parallel
LD, RD, PD, BD = 3, 16, 20, 4


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_data():
    from oracle import unet_oracle as U
    from road_segmentation_unet_amd.unet import input_size_needed
    rng = np.random.RandomState(12)
    S = input_size_needed(PD, LD)
    X = rng.rand(2, BD, S, S, 3).astype(f32)
    labels = (rng.rand(2, BD, PD, PD) < 0.3).astype(np.float64)
    return X, labels, U.init_params(LD, RD, True, seed=13, bias_scale=0.05)


def _dp_model(params, eps):
    from road_segmentation_unet_amd.model import ConvolutionalModel, Options
    return ConvolutionalModel(Options(num_layers=LD, root_size=RD, patch_size=PD, batch_size=BD, dilated_layers=True, dropout=1.0, lr=0.01,
                                      seed=3, optimizer="adam", adam_epsilon=eps), device="cuda:0", params=params)


def _dp_steps(model, X, labels, sl, eps):
    """two steps; each checked against the numpy ApplyAdam of the gradient the step used (flat_g after the all-reduce)"""
    net, n = model.net, model.net.n_live
    b1p, b2p = f32(0.9), f32(0.999)
    for step in range(2):
        torch.cuda.synchronize()
        w0, m0, v0 = (x[:n].cpu().numpy() for x in (net.flat_w, net.flat_acc, net.flat_v))
        gs = net.global_step
        model.train_step(X[step][sl], labels[step][sl])
        torch.cuda.synchronize()
        g = net.flat_g[:n].cpu().numpy()
        rw, rm, rv = np_adam(w0, m0, v0, g, tf_alpha(0.01, gs, b1p, b2p), 0.9, 0.999, eps)
        assert_close_ulp(net.flat_w[:n].cpu().numpy(), rw, "w step %d" % step)
        assert_close_ulp(net.flat_acc[:n].cpu().numpy(), rm, "m step %d" % step)
        assert_close_ulp(net.flat_v[:n].cpu().numpy(), rv, "v step %d" % step)
        b1p, b2p = b1p * f32(0.9), b2p * f32(0.999)
    return {k: v for k, v in net.state_dict().items() if k != "global_step"}


def _dp_worker(rank, world, port, eps, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LOCAL_RANK="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        X, labels, params = _dp_data()
        m = _dp_model(params, eps)
        assert m.world == world and m.local_batch == BD // world
        per = BD // world
        q.put((rank, _dp_steps(m, X, labels, slice(rank * per, (rank + 1) * per), eps)))
    except Exception as e:   # (the parent must not wait for a result that never comes)
        q.put((rank, repr(e)))
        raise
    finally:
        dist.destroy_process_group()


def test_adam_two_rank_steps():
    """two gloo ranks on one GPU (the pattern of test_gpu_dp.py), optimizer adam: the ranks stay bit-identical in w, m and v, each rank's
    steps are the numpy Adam of its reduced gradient, and the result agrees with one process stepping on the whole batch"""
    from road_segmentation_unet_amd.unet import UNet
    X, labels, params = _dp_data()
    # epsilon near the gradients' RMS: with epsilon << |g| the first steps are ~lr * sign(g), and a gradient element near zero whose
    # sign flips with the fp32 summation order (two 2-patch partial sums against one 4-patch sum) would move by 2 lr; with epsilon ~ RMS(g)
    # the step is smooth in g and the order difference stays a tiny fraction of the update
    probe = UNet(LD, RD, True, BD, PD, params=params, training=True, optimizer="adam")
    probe.x.copy_(torch.from_numpy(X[0])); probe.labels.copy_(torch.from_numpy(labels[0]).to(torch.int64))
    probe.forward_device()
    probe.backward_device(1.0 / (BD * PD * PD))
    eps = float(torch.sqrt(torch.mean(probe.flat_g[:probe.n_live] ** 2)).item())
    del probe
    assert eps > 0
    single = _dp_model(params, eps)
    ref = _dp_steps(single, X, labels, slice(0, BD), eps)
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, eps, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(2)]
    got = dict(res)
    assert all(isinstance(v, dict) for v in got.values()), got
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for k in ref:
        np.testing.assert_array_equal(got[0][k], got[1][k], err_msg="ranks diverged: " + k)
    for n in single.net.names:
        upd = np.abs(ref[n] - params[n]).max()
        if upd == 0:
            continue
        # stated tolerance: 2 % of the tensor's largest update (the same bound test_gpu_dp.py states for Momentum)
        assert np.abs(got[0][n] - ref[n]).max() <= 2e-2 * upd + 1e-7, (n, float(np.abs(got[0][n] - ref[n]).max()), float(upd))


# ------------------------------------------------------------------------------------------- command line
def test_cli_trains_with_adam(tmp_path, capsys):
    from PIL import Image
    from road_segmentation_unet_amd.cli import main
    rng = np.random.RandomState(4)
    tr = tmp_path / "train"
    (tr / "images").mkdir(parents=True)
    (tr / "groundtruth").mkdir(parents=True)
    H = 48
    for i in range(3):
        img = (rng.rand(H, H, 3) * 255).astype(np.uint8)
        gt = ((img[..., 0] > 127) * 255).astype(np.uint8)
        Image.fromarray(img).save(tr / "images" / ("satImage_%03d.png" % i))
        Image.fromarray(gt).save(tr / "groundtruth" / ("satImage_%03d.png" % i))
    save = tmp_path / "runs"
    argv = ["--num_layers=2", "--root_size=16", "--patch_size=16", "--stride=16", "--batch_size=4", "--num_epoch=1", "--lr=0.001",
            "--optimizer=adam", "--train_data_dir=%s" % tr, "--save_path=%s" % save, "--logdir=%s" % (tmp_path / "logs"),
            "--rotation_angles=0,90", "--seed=5"]
    assert main(argv) == 0
    out = capsys.readouterr().out
    losses = re.findall(r"'loss': ([^,}]+)", out)
    assert losses and all(np.isfinite(float(x)) for x in losses), out[-2000:]
    runs = [d for d in os.listdir(save) if os.path.isdir(save / d)]
    ck = [f for f in os.listdir(save / runs[0]) if f.endswith(".npz")]
    assert len(ck) == 1
    with np.load(save / runs[0] / ck[0]) as z:
        keys = set(z.files)
    assert "conv_0|conv1|kernel|Adam" in keys and "conv_0|conv1|kernel|Adam_1" in keys and "beta1_power" in keys
    assert not any(k.endswith("|Momentum") for k in keys)


# ------------------------------------------------------------------------------------------- it trains
def test_adam_lowers_the_loss_on_a_fixed_batch():
    """thirty Adam steps at lr 1e-3 on one fixed batch (labels: the red channel above 0.5 -- learnable) lower the loss by >= 30 %"""
    from oracle import unet_oracle as U
    from road_segmentation_unet_amd.unet import UNet, input_size_needed
    L, root, P, B = 2, 16, 20, 4
    S = input_size_needed(P, L)
    rng = np.random.RandomState(21)
    X = rng.rand(B, S, S, 3).astype(f32)
    off = (S - P) // 2
    labels = (X[:, off:off + P, off:off + P, 0] > 0.5).astype(np.int64)
    m = UNet(L, root, False, B, P, params=U.init_params(L, root, False, seed=5, bias_scale=0.0), training=True, optimizer="adam")
    m.x.copy_(torch.from_numpy(X))
    m.labels.copy_(torch.from_numpy(labels))
    losses = []
    for _ in range(31):
        m.forward_device()
        m.backward_device(1.0 / (B * P * P))
        losses.append(float(m.loss_sum.item()) / (B * P * P))
        m.apply_adam(1e-3)
    assert all(np.isfinite(losses))
    assert losses[30] <= 0.7 * losses[0], losses
