"""-m gpu: gradient accumulation -- the device pass (rsu_grad_accumulate) bit for bit against its numpy float32 restatement
(tests/accum_util.py); the accumulating net beside a plain twin that is handed the host sum of the same gradients; the driver against
one big batch, in one process and over two gloo ranks; dropout masks per micro-batch; the command line.
Bit equality everywhere except against the big batch, where only the float32 summation order differs: there the tolerance is the one
tests/test_gpu_dp.py states for the same situation (partial sums of a split batch against one sum)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from road_segmentation_unet_amd import optim as optim_mod
from road_segmentation_unet_amd import unet as unet_mod
from road_segmentation_unet_amd._lib import RsuError, call
from road_segmentation_unet_amd.unet import UNet, ema_decay_at
from tests import accum_util as au
from tests.accum_util import same

pytestmark = pytest.mark.gpu

f32 = np.float32
DEV = "cuda:0"
PAD = 64                                   # floats in front of and behind a slice: 256 bytes, so the slice stays 16-byte aligned
SHARE = 8192                               # floats per workgroup of the pass (rsu.h RSU_GRAD_ACCUMULATE_BLOCK_FLOATS)
NS = [1, 3, 4, 5, 1023, 1024, SHARE, SHARE + 5, 2 * SHARE + 7, 3 * 16384 + 1]


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Slices:
    """dst[0:n) and src[0:n) as slices of two larger buffers of random floats"""

    def __init__(self, n, seed):
        rng = np.random.RandomState(seed)
        self.n = n
        self.big_d = torch.from_numpy(rng.randn(n + 2 * PAD).astype(f32)).to(DEV)
        self.big_s = torch.from_numpy(rng.randn(n + 2 * PAD).astype(f32)).to(DEV)
        self.d, self.s = self.big_d[PAD:PAD + n], self.big_s[PAD:PAD + n]
        assert self.d.data_ptr() % 16 == 0 and self.s.data_ptr() % 16 == 0

    def run(self, assign):
        call("rsu_grad_accumulate", self.d.data_ptr(), self.s.data_ptr(), self.n, int(assign), _stream())
        torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------- 1. the kernel
def test_share_constant():
    from road_segmentation_unet_amd import _lib
    assert SHARE == _lib.GRAD_ACCUMULATE_BLOCK_FLOATS


@pytest.mark.parametrize("assign", [0, 1])
@pytest.mark.parametrize("n", NS)
def test_pass_equals_the_float32_restatement(n, assign):
    s = Slices(n, 200 + n % 991)
    d0, s0 = s.big_d.cpu().numpy().copy(), s.big_s.cpu().numpy().copy()
    s.run(assign)
    d1 = s.big_d.cpu().numpy()
    assert same(d1[PAD:PAD + n], au.host_accumulate(d0[PAD:PAD + n], s0[PAD:PAD + n], assign))
    assert same(d1[:PAD], d0[:PAD]) and same(d1[PAD + n:], d0[PAD + n:]), "written outside dst[0, n)"
    assert same(s.big_s, s0), "src was written"


@pytest.mark.parametrize("n", [5, SHARE + 5, 3 * 16384 + 1])
def test_assign_does_not_read_dst(n):
    """dst pre-filled with nan: after an assign no nan is left, and dst is src"""
    s = Slices(n, 11)
    s.d.fill_(float("nan"))
    s.run(1)
    out = s.d.cpu().numpy()
    assert not np.isnan(out).any() and same(out, s.s)


@pytest.mark.parametrize("n", [7, SHARE + 5])
def test_inf_nan_and_negative_zero_follow_ieee(n):
    s = Slices(n, 12)
    special = np.array([np.inf, -np.inf, np.nan, -0.0, 0.0, 1.0, 3e38], f32)
    rng = np.random.RandomState(13)
    d0, s0 = special[rng.randint(0, 7, n)], special[rng.randint(0, 7, n)]
    d0[:7], s0[:7] = special, special[[1, 1, 5, 3, 3, 2, 6]]   # inf - inf, -inf - inf, nan + 1, -0 + -0, 0 + -0, 1 + nan, 3e38 + 3e38
    s.d.copy_(torch.from_numpy(d0))
    s.s.copy_(torch.from_numpy(s0))
    s.run(0)
    got, want = s.d.cpu().numpy(), au.host_accumulate(d0, s0, False)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = ~np.isnan(want)
    assert same(got[ok], want[ok])                                # signed zeros and infinities included: the bits
    assert np.isnan(got[0]) and got[1] == -np.inf and np.isnan(got[2]) and np.signbit(got[3]) and not np.signbit(got[4]) and got[6] == np.inf
    s.run(1)                                                      # an assign copies the specials, payloads and signs included
    assert np.array_equal(au.bits(s.d), au.bits(s0))


def test_three_chained_calls_sum_left_to_right():
    n = 2 * SHARE + 7
    rng = np.random.RandomState(14)
    a, b, c = [(rng.randn(n) * 10.0 ** rng.randint(-3, 4, n)).astype(f32) for _ in range(3)]
    a[:3], b[:3], c[:3] = f32(2.0 ** 24), f32(1.0), f32(1.0)     # (a + b) + c = 2^24, a + (b + c) = 2^24 + 2
    s = Slices(n, 15)
    for k, (src, assign) in enumerate(((a, 1), (b, 0), (c, 0))):
        s.s.copy_(torch.from_numpy(src))
        s.run(assign)
        assert same(s.d, au.host_sum([a, b, c][:k + 1])), "call %d" % k
    assert float(s.d[0]) == 2.0 ** 24
    want = ((a + b).astype(f32) + c).astype(f32)
    assert same(s.d, want) and not same(s.d, (a + (b + c).astype(f32)).astype(f32))


def test_argument_checks_raise():
    s = Slices(64, 16)
    d0 = s.big_d.clone()
    d, src, st = s.d.data_ptr(), s.s.data_ptr(), _stream()
    for assign in (0, 1):
        for args in ((None, src, 64), (d, None, 64),                     # NULL pointers
                     (d, src, 0), (d, src, -1),                          # n < 1
                     (d + 4, src, 32), (d, src + 8, 32),                 # a pointer not 16-byte aligned
                     (d, d, 64), (d, d + 16, 64), (d + 16, d, 32)):      # overlapping ranges
            with pytest.raises(RsuError):
                call("rsu_grad_accumulate", args[0], args[1], args[2], assign, st)
    torch.cuda.synchronize()
    assert same(s.big_d, d0)


# ------------------------------------------------------------------------------------------- 2. the network
P, B, K = 20, 2, 3


def _batches(net, k, seed, b=B):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    return [(torch.rand((b, net.S, net.S, 3), generator=gen), (torch.rand((b, P, P), generator=gen) < 0.3).to(torch.int64)) for _ in range(k)]


def _passes(m, x, y, inv, keep=1.0):
    m.x.copy_(x); m.labels.copy_(y)
    m.forward_device(keep=keep)
    m.backward_device(inv)


def _apply(m):
    m.apply_adam(0.01) if m.optimizer == "adam" else m.apply_momentum(0.01, 0.9)
    torch.cuda.synchronize()


def _slots_equal(a, b):
    assert same(a.flat_w, b.flat_w) and same(a.flat_acc, b.flat_acc)
    assert (a.flat_v is None) == (b.flat_v is None)
    if a.flat_v is not None:
        assert same(a.flat_v, b.flat_v)
    assert set(a.pk) == set(b.pk)
    for k in a.pk:
        assert torch.equal(a.pk[k].view(torch.int16), b.pk[k].view(torch.int16)), k


@pytest.mark.parametrize("optimizer", ["momentum", "adam"])
@pytest.mark.parametrize("L,dilated", [(2, False), (3, True)])
def test_accumulating_net_beside_a_twin(L, dilated, optimizer):
    """after the K-th accumulate_gradients() flat_g is the float32 host sum, in the stated order, of the gradients a plain twin computes
    for the same micro-batches; stepping the twin on that sum gives the accumulating net's weights, slots and packed copies bit for
    bit -- twice: the second step shows that the assign of micro-step 0 forgets the first step's sum"""
    net = UNet(L, 16, dilated, B, P, seed=41, optimizer=optimizer, accumulate_steps=K)
    twin = UNet(L, 16, dilated, B, P, seed=41, optimizer=optimizer)
    assert net.accumulate_steps == K and twin.accumulate_steps == 1 and twin.flat_gsum is None
    assert net.flat_gsum.dtype == torch.float32 and net.flat_gsum.numel() == net.n_flat and not net.flat_gsum.any()
    inv = 1.0 / (K * B * P * P)
    batches = _batches(net, 2 * K, 42)
    for step in (1, 2):
        grads = []
        for j in range(K):
            assert net.micro_step == j and twin.micro_step == 0
            x, y = batches[(step - 1) * K + j]
            _passes(net, x, y, inv)
            net.accumulate_gradients()
            _passes(twin, x, y, inv)
            torch.cuda.synchronize()
            grads.append(twin.flat_g.cpu().numpy().copy())
            if j < K - 1:
                w0 = net.flat_w.clone()
                with pytest.raises(RsuError, match="accumulate_gradients"):
                    _apply(net)                                   # after 1 and after 2 of 3 calls
                assert net.global_step == step - 1 and same(net.flat_w, w0)
        want = au.host_sum(grads)
        assert not same(want, grads[-1])
        assert same(net.flat_g, want), "step %d: flat_g is not ((g_0 + g_1) + g_2)" % step
        with pytest.raises(RsuError, match="apply_"):
            net.accumulate_gradients()                            # a fourth call without a step
        twin.flat_g.copy_(torch.from_numpy(want))
        _apply(net)
        _apply(twin)
        _slots_equal(net, twin)
        assert net.global_step == twin.global_step == step and net.micro_step == 0


def test_arguments_and_the_net_that_does_not_accumulate(monkeypatch):
    for bad in (0, -1, 2.0, "2", True, float("nan")):
        with pytest.raises(RsuError):
            UNet(2, 16, False, B, P, accumulate_steps=bad)
    with pytest.raises(RsuError):
        UNet(2, 16, False, B, P, training=False, accumulate_steps=2)
    assert UNet(2, 16, False, B, P, training=False, accumulate_steps=1).flat_gsum is None
    names = []
    real = unet_mod.call
    for mod in (unet_mod, optim_mod):   # (the passes' calls and the optimizer step's)
        monkeypatch.setattr(mod, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    one = UNet(2, 16, False, B, P, seed=43, accumulate_steps=1)
    none = UNet(2, 16, False, B, P, seed=43, accumulate_steps=None)
    plain = UNet(2, 16, False, B, P, seed=43)
    inv = 1.0 / (B * P * P)
    for x, y in _batches(plain, 2, 44):
        for m in (one, none, plain):
            assert m.flat_gsum is None and m.micro_step == 0 and m.accumulate_steps == 1
            _passes(m, x, y, inv)
            if m is not plain:
                m.accumulate_gradients()                          # nothing: no launch, no count
            _apply(m)
        _slots_equal(one, plain)
        _slots_equal(none, plain)
        assert same(one.flat_g, plain.flat_g)
    assert one.global_step == plain.global_step == 2
    assert "rsu_grad_accumulate" not in names and "rsu_head_fwd_bwd" in names


@pytest.mark.parametrize("optimizer", ["momentum", "adam"])
def test_an_inf_in_micro_step_0_skips_the_whole_step(optimizer):
    """clip_grad_norm=1e30 only measures and guards: the inf travels through the sum into flat_g, where rsu_grad_norm sees it"""
    net = UNet(2, 16, False, B, P, seed=45, optimizer=optimizer, clip_grad_norm=1e30, accumulate_steps=K)
    inv = 1.0 / (K * B * P * P)
    w0, acc0 = net.flat_w.clone(), net.flat_acc.clone()
    pk0 = {k: t.clone() for k, t in net.pk.items()}
    for j, (x, y) in enumerate(_batches(net, K, 46)):
        _passes(net, x, y, inv)
        if j == 0:
            net.g["conv_1/conv1/kernel"].view(-1)[7] = float("inf")
        net.accumulate_gradients()
    _apply(net)
    stats = net.clip_stats()
    assert stats["skipped"] == 1 and stats["last_skipped"] and stats["steps"] == 1
    assert same(net.flat_w, w0) and same(net.flat_acc, acc0)
    for k in pk0:
        assert torch.equal(net.pk[k].view(torch.int16), pk0[k].view(torch.int16)), k
    assert net.global_step == 1 and net.micro_step == 0          # the step still counts (see UNet.apply_momentum)
    for x, y in _batches(net, K, 47):                             # the next step forgets the inf: the assign of micro-step 0
        _passes(net, x, y, inv)
        net.accumulate_gradients()
    _apply(net)
    assert net.clip_stats()["skipped"] == 1 and not same(net.flat_w, w0) and np.isfinite(net.flat_g.cpu().numpy()).all()


def test_averages_move_once_per_optimizer_step():
    from tests.test_gpu_ema import host_ema
    net = UNet(2, 16, False, B, P, seed=48, ema_decay=0.9, accumulate_steps=K)
    inv = 1.0 / (K * B * P * P)
    e, n = net.flat_w.cpu().numpy().copy(), net.n_live
    batches = _batches(net, 2 * K, 49)
    for t in (1, 2):
        for j in range(K):
            _passes(net, *batches[(t - 1) * K + j], inv)
            net.accumulate_gradients()
            torch.cuda.synchronize()
            assert same(net.flat_ema, e), "the averages moved inside step %d" % t
        _apply(net)
        e[:n] = host_ema(e[:n], net.flat_w.cpu().numpy()[:n], f32(1) - ema_decay_at(0.9, t, True))
        assert same(net.flat_ema, e), "step %d" % t


# ------------------------------------------------------------------------------------------- 5. dropout
def test_micro_batches_of_one_step_draw_different_masks():
    net = UNet(2, 16, False, B, P, seed=50, accumulate_steps=2)
    x, y = _batches(net, 1, 51)[0]
    inv = 1.0 / (2 * B * P * P)
    g = []
    for keep in (1.0, 0.8):
        for j in range(2):
            assert net.micro_step == j
            _passes(net, x, y, inv, keep=keep)
            torch.cuda.synchronize()
            g.append(net.flat_g.clone())
            net.accumulate_gradients()
        net._accum_calls = 0                                      # (no step between the two rounds: the weights stay, so only the masks can differ)
    assert same(g[0], g[1]), "without dropout identical data must give identical gradients"
    assert not same(g[2], g[3]), "the two micro-batches drew the same masks"
    assert not same(g[2], g[0])
    assert net.dropout_key(1) == au.host_dropout_key(50, 1, 0, 0)
    net._accum_calls = 1
    assert net.dropout_key(1) == au.host_dropout_key(50, 1, 0, 1) != au.host_dropout_key(50, 1, 0, 0)


def test_first_dropout_step_of_a_k1_net_is_the_plain_nets():
    one, plain = UNet(2, 16, False, B, P, seed=52, accumulate_steps=1), UNet(2, 16, False, B, P, seed=52)
    x, y = _batches(plain, 1, 53)[0]
    for m in (one, plain):
        _passes(m, x, y, 1.0 / (B * P * P), keep=0.8)
        m.accumulate_gradients()
        _apply(m)
    assert same(one.flat_g, plain.flat_g)
    _slots_equal(one, plain)


# ------------------------------------------------------------------------------------------- 3. the driver against the big batch
LD, ROOT = 3, 16


def _data(batch):
    from oracle import unet_oracle as U
    S = U.input_size_needed(P, LD)
    rng = np.random.RandomState(60)
    X = rng.rand(2, batch, S, S, 3).astype(f32)
    labels = (rng.rand(2, batch, P, P) < 0.3).astype(np.float64)
    params = U.init_params(LD, ROOT, True, seed=61, bias_scale=0.05)
    return X, labels, params


def _options(batch, **kw):
    from road_segmentation_unet_amd.model import Options
    o = dict(num_layers=LD, root_size=ROOT, patch_size=P, batch_size=batch, dilated_layers=True, dropout=1.0, lr=0.05, seed=3, logdir=None)
    o.update(kw)
    return Options(**o)


def _steps(model, X, labels, sl):
    out = []
    for step in range(2):
        loss, pred = model.train_step(X[step][sl], labels[step][sl])
        out.append((float(loss), tuple(pred.shape), pred.detach().cpu().numpy().copy()))
    torch.cuda.synchronize()
    sd = model.net.state_dict()
    return {k: v for k, v in sd.items() if not k.endswith("/Momentum") and k != "global_step"}, out, int(sd["global_step"])


def _assert_close_to_big_batch(got, ref, params):
    """|w_acc - w_ref| <= 2e-2 * max|w_ref - w_init| + 1e-7 per variable: bf16 activations identical, only the fp32 order of the sum over the
    batch differs (tests/test_gpu_dp.py)"""
    for n in ref:
        upd = np.abs(ref[n] - params[n]).max()
        if upd == 0:
            continue
        err = float(np.abs(got[n] - ref[n]).max())
        assert err <= 2e-2 * upd + 1e-7, (n, err, float(upd))


@pytest.mark.parametrize("extra", [{}, {"dice_weight": 0, "class_weights": "1,3"}], ids=["plain", "class_weights"])
def test_two_micro_batches_equal_one_big_batch(extra):
    from road_segmentation_unet_amd.model import ConvolutionalModel
    X, labels, params = _data(4)
    acc = ConvolutionalModel(_options(4, accumulate_steps=2, **extra), device=DEV, params=params)
    big = ConvolutionalModel(_options(4, **extra), device=DEV, params=params)
    assert acc.local_batch == 2 and acc.net.B == 2 and acc.net.accumulate_steps == 2 and big.local_batch == 4 and big.net.flat_gsum is None
    w_acc, out_acc, gs_acc = _steps(acc, X, labels, slice(0, 4))
    w_big, out_big, gs_big = _steps(big, X, labels, slice(0, 4))
    assert gs_acc == gs_big == 2                                  # optimizer steps, not micro-batches
    for (la, sa, pa), (lb, sb, pb) in zip(out_acc, out_big):
        assert sa == sb == (4, P, P)
        assert abs(la - lb) <= 1e-5 * abs(lb), (la, lb)
    # step 1's predictions come from identical weights: per-patch arithmetic does not depend on the batch it sits in
    np.testing.assert_allclose(out_acc[0][2], out_big[0][2], rtol=0, atol=1e-6)
    _assert_close_to_big_batch(w_acc, w_big, params)
    with pytest.raises(ValueError, match="whole share"):
        acc.train_step(X[0][:2], labels[0][:2])


# ------------------------------------------------------------------------------------------- 4. two gloo ranks on cuda:0
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), LOCAL_RANK="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from road_segmentation_unet_amd.model import ConvolutionalModel
        X, labels, params = _data(8)
        m = ConvolutionalModel(_options(8, accumulate_steps=2), device=DEV, params=params)
        assert m.world == world and m.local_batch == 2 and m.net.on_grads is None and m._bucketer is not None
        per = 8 // world
        w, out, gs = _steps(m, X, labels, slice(rank * per, (rank + 1) * per))
        q.put((rank, w, [(o[0], o[1]) for o in out], gs, m.exchange_schedule))
    finally:
        dist.destroy_process_group()


def test_two_ranks_times_two_micro_batches_equal_one_process():
    from road_segmentation_unet_amd.model import ConvolutionalModel
    X, labels, params = _data(8)
    single = ConvolutionalModel(_options(8), device=DEV, params=params)
    ref, out_ref, _ = _steps(single, X, labels, slice(0, 8))
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in range(2)]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    got = {r[0]: r for r in res}
    for r in res:
        assert r[3] == 2 and r[4] is None                         # two optimizer steps; the exchange schedule was not tuned
        for (loss, shape), (lref, _, _) in zip(r[2], out_ref):
            assert shape == (4, P, P) and abs(loss - lref) <= 1e-5 * abs(lref), (loss, lref)
    for n in ref:
        np.testing.assert_array_equal(got[0][1][n], got[1][1][n], err_msg="ranks diverged: " + n)   # replicas stay identical
    _assert_close_to_big_batch(got[0][1], ref, params)


# ------------------------------------------------------------------------------------------- 6. the command line
@pytest.mark.parametrize("pool_flag", ["--device_patch_pool", "--nodevice_patch_pool"])
def test_cli_counts_optimizer_steps(tmp_path, pool_flag):
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
    argv = ["--num_layers=2", "--root_size=16", "--patch_size=16", "--stride=16", "--batch_size=4", "--accumulate_steps=2", "--num_epoch=1",
            "--lr=0.001", "--train_data_dir=%s" % tr, "--save_path=%s" % runs, "--logdir=%s" % (tmp_path / "logs"), "--rotation_angles=0,90",
            "--seed=5", pool_flag]
    assert main(argv) == 0
    files = sorted(runs.rglob("model-epoch-000.chkpt.npz"))
    assert len(files) == 1
    with np.load(str(files[0])) as z:
        assert int(z["global_step"]) == len(range(0, 72 - 4, 4)) == 17   # optimizer steps over 72 patches, not micro-batches
        assert np.isfinite(z["conv_0|conv1|kernel"]).all()
