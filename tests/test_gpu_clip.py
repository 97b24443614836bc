"""-m gpu: global-norm gradient clipping with the device-side guard against a gradient that is not finite -- the norm kernel
(rsu_grad_norm) on exactly summable and on random values, its flags and counters, the clipping update passes
(rsu_update_table_run_clip / _adam_clip) bit for bit against the plain passes with the same scale as gscale, the skipped step, the
untouched default step, and the model / command-line surface."""
import json
import os
import re

import numpy as np
import pytest
import torch

from road_segmentation_unet_amd import _lib
from road_segmentation_unet_amd._lib import RsuError, call, lib
from road_segmentation_unet_amd.unet import UNet, clip_scale

pytestmark = pytest.mark.gpu

f32 = np.float32
SHARE = _lib.GRAD_NORM_BLOCK_FLOATS    # floats of g per workgroup of pass 1
LANE_ROW = 256 * 4                     # one float4 per lane of a workgroup
NAN_BITS = 0x7FC12345                  # the sentinel behind the workspace (a quiet nan with a payload no kernel produces)
SLACK = 64


def _stream():
    return torch.cuda.current_stream().cuda_stream


class Norm:
    """g[0:n) in a buffer whose floats behind n are nan (a read of them poisons the sum and raises the flag), a workspace with a sentinel
    behind rsu_grad_norm_ws_floats(n) floats, and a zeroed state record"""

    def __init__(self, values):
        n = self.n = int(values.shape[0])
        self.g = torch.full((n + SLACK,), float("nan"), device="cuda:0")
        self.g[:n] = torch.from_numpy(values).cuda()
        self.nws = lib().rsu_grad_norm_ws_floats(n)
        self.ws = torch.full((self.nws + SLACK,), NAN_BITS, dtype=torch.int32, device="cuda:0")
        self.state = torch.zeros(8, dtype=torch.int32, device="cuda:0")

    def run(self, max_norm):
        call("rsu_grad_norm", self.g.data_ptr(), self.n, max_norm, self.ws.data_ptr(), self.state.data_ptr(), _stream())
        torch.cuda.synchronize()
        raw = self.state.cpu().numpy()
        fl = raw.view(f32)
        return {"sumsq": fl[0], "norm": fl[1], "scale": fl[2], "flags": int(raw[3]), "steps": int(raw[4]), "clipped": int(raw[5]),
                "skipped": int(raw[6]), "pad": int(raw[7])}

    def check_ws(self):
        ws = self.ws.cpu().numpy()
        assert np.all(ws[self.nws:] == NAN_BITS), "the workspace was written behind rsu_grad_norm_ws_floats(n)"
        assert not np.any(ws[:self.nws] == NAN_BITS), "a workgroup left its partial unwritten"


# ------------------------------------------------------------------------------------------- 1. exact norm
@pytest.mark.parametrize("n", [1, 3, 4, 5, LANE_ROW, SHARE, SHARE + 1, 2 * SHARE - 1, (1 << 20) + 3])
def test_norm_is_exact_on_small_integers(n):
    """g in {-1, 0, 1}: the sum of squares is an integer below 2^24, exact in float32 in any order, so sumsq is the count of non-zeros
    and norm / scale are clip_scale of it bit for bit; nothing behind g[n) enters, nothing behind the workspace is written; a second
    call gives the same record and the counters advance"""
    rng = np.random.RandomState(1000 + n % 997)
    vals = rng.randint(-1, 2, size=n).astype(f32)
    vals[n - 1] = 1.0   # (the last element, in the scalar tail when n & 3, always counts)
    count = int(np.count_nonzero(vals))
    t = Norm(vals)
    c = 3.0
    a = t.run(c)
    t.check_ws()
    assert a["sumsq"] == f32(count)
    norm, scale = clip_scale(f32(count), c)
    assert a["norm"].tobytes() == norm.tobytes() and a["scale"].tobytes() == scale.tobytes()
    clipped = count > 9
    assert a["flags"] == (_lib.CLIP_CLIPPED if clipped else 0) and (a["scale"] < 1) == clipped
    assert (a["steps"], a["clipped"], a["skipped"], a["pad"]) == (1, int(clipped), 0, 0)
    b = t.run(c)
    for k in ("sumsq", "norm", "scale"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert b["flags"] == a["flags"] and (b["steps"], b["clipped"], b["skipped"]) == (2, 2 * int(clipped), 0)
    d = t.run(1e30)   # a huge bound only measures
    assert d["sumsq"] == f32(count) and d["scale"] == 1 and d["flags"] == 0
    assert (d["steps"], d["clipped"], d["skipped"]) == (3, 2 * int(clipped), 0)
    t.check_ws()


# ------------------------------------------------------------------------------------------- 2. random values
def test_norm_of_random_values_within_the_summation_bound():
    """randn * 1e-3 at n = 2^20 + 3 against float64 numpy. The bound follows the summation that was built: every term g^2 passes
    through at most 29 float32 roundings -- 1 for the square, 16 in its lane's chain (16 float4 per lane, one chain per component), 2 to
    join the four chains, 1 for the scalar tail's term (lanes 0..2 of workgroup 0 only), 6 levels of the wave's tree, 2 to join the four
    waves, and 1 when the double sum of the partials is rounded to the record's float; the double sum itself adds (partials / 256 + 8)
    * 2^-53, covered by the 2^-40 below. All terms are >= 0, so the relative error of sumsq is at most gamma_29 = 29 u / (1 - 29 u),
    u = 2^-24: 1.73e-6. norm = (float)sqrt(sumsq): the square root halves it and the conversion adds one rounding: (29 / 2 + 1) u."""
    n = (1 << 20) + 3
    rng = np.random.RandomState(7)
    vals = (rng.randn(n) * 1e-3).astype(f32)
    ref = float(np.sum(vals.astype(np.float64) ** 2))
    t = Norm(vals)
    r = t.run(0.5)
    t.check_ws()
    u = 2.0 ** -24
    tol_sumsq = 29 * u / (1 - 29 * u) + 2.0 ** -40
    tol_norm = (29 / 2 + 1) * u / (1 - 29 * u) + 2.0 ** -40
    err_sumsq = abs(float(r["sumsq"]) - ref) / ref
    err_norm = abs(float(r["norm"]) - np.sqrt(ref)) / np.sqrt(ref)
    print("sumsq rel err %.3e (bound %.3e), norm rel err %.3e (bound %.3e)" % (err_sumsq, tol_sumsq, err_norm, tol_norm))
    assert err_sumsq <= tol_sumsq and err_norm <= tol_norm
    norm, scale = clip_scale(r["sumsq"], 0.5)   # norm ~ 1.02 > 0.5: clipped
    assert r["norm"].tobytes() == norm.tobytes() and r["scale"].tobytes() == scale.tobytes() and r["flags"] == _lib.CLIP_CLIPPED
    again = t.run(0.5)
    assert again["sumsq"].tobytes() == r["sumsq"].tobytes()


# ------------------------------------------------------------------------------------------- 3. values that are not finite
def test_values_that_are_not_finite_raise_the_flag():
    """one nan in the scalar tail, one inf in the first float4, one 1e30 (finite; its square overflows) in the middle: each sets bit 1,
    scale 0 and skipped_steps + 1; a clean gradient afterwards clears the flag (ordinary loads of special values)"""
    n = 2 * SHARE + 3
    rng = np.random.RandomState(3)
    base = rng.randint(-1, 2, size=n).astype(f32)
    t = Norm(base)
    clean = t.run(1e30)
    assert clean["flags"] == 0 and clean["scale"] == 1 and clean["skipped"] == 0
    for k, (pos, val) in enumerate(((n - 1, float("nan")), (1, float("inf")), (n // 2, 1e30))):
        assert not (pos == n - 1) or (n & 3 and pos >= (n >> 2) << 2)
        t.g[:n] = torch.from_numpy(base).cuda()
        t.g[pos] = val
        r = t.run(1e30)
        assert r["flags"] == _lib.CLIP_NONFINITE and r["scale"] == 0 and not np.isfinite(r["sumsq"]), (pos, r)
        assert (r["steps"], r["clipped"], r["skipped"]) == (2 + k, 0, 1 + k)
    t.g[:n] = torch.from_numpy(base).cuda()
    r = t.run(1e30)
    assert r["flags"] == 0 and r["scale"] == 1 and r["sumsq"].tobytes() == clean["sumsq"].tobytes()
    assert (r["steps"], r["skipped"]) == (5, 3)
    t.check_ws()


# ------------------------------------------------------------------------------------------- 4. / 5. the update passes
def _power(beta, t):
    p = f32(beta)
    for _ in range(t - 1):
        p = f32(p * f32(beta))
    return p


class Pair:
    """a clipping net and a non-clipping twin from the same parameters, holding the same gradient (a real forward + backward of the twin)
    and the same non-zero optimizer slots"""

    def __init__(self, L, root, dilated, P, optimizer, B=2):
        self.opt = optimizer
        self.twin = UNet(L, root, dilated, B, P, seed=17, training=True, optimizer=optimizer)
        self.net = UNet(L, root, dilated, B, P, seed=17, training=True, optimizer=optimizer, clip_grad_norm=1.0)
        assert torch.equal(self.net.flat_w, self.twin.flat_w)
        gen = torch.Generator(device="cpu").manual_seed(6)
        t = self.twin
        t.x.copy_(torch.rand((B, t.S, t.S, 3), generator=gen))
        t.labels.copy_((torch.rand((B, P, P), generator=gen) < 0.3).to(torch.int64))
        t.forward_device()
        t.backward_device(1.0 / (B * P * P))
        torch.cuda.synchronize()
        n = self.n = t.n_live
        self.grad = t.flat_g.clone()
        self.norm64 = float(np.sqrt(np.sum(self.grad[:n].cpu().numpy().astype(np.float64) ** 2)))
        assert np.isfinite(self.norm64) and self.norm64 > 0
        self.w0 = t.flat_w.clone()
        self.acc0 = torch.zeros_like(t.flat_w)
        self.acc0[:n] = torch.randn(n, generator=gen).cuda() * 1e-3
        self.v0 = torch.zeros_like(t.flat_w)
        self.v0[:n] = torch.rand(n, generator=gen).cuda() * 1e-6

    def restore(self, m, like=None):
        """the start state on net m: weights, slots, packed copies, the gradient; step and powers 5 steps in, or those of `like`"""
        m.flat_w.copy_(self.w0); m.flat_acc.copy_(self.acc0); m.flat_g.copy_(self.grad)
        if self.opt == "adam":
            m.flat_v.copy_(self.v0)
        if like is None:
            m.global_step = 5
            m.beta1_power, m.beta2_power = (_power(0.9, 6), _power(0.999, 6)) if self.opt == "adam" else (None, None)
        else:
            m.global_step, m.beta1_power, m.beta2_power = like
        m.repack()

    def step(self, m, gscale=1.0):
        if self.opt == "adam":
            m.apply_adam(0.01, 0.9, 0.999, 1e-8, gscale=gscale)
        else:
            m.apply_momentum(0.01, 0.9, gscale=gscale)
        torch.cuda.synchronize()

    @staticmethod
    def snapshot(m):
        return {"w": m.flat_w.clone(), "acc": m.flat_acc.clone(), "v": None if m.flat_v is None else m.flat_v.clone(),
                "pk": {k: t.clone() for k, t in m.pk.items()}}

    @staticmethod
    def assert_same(a, b, what):
        assert torch.equal(a["w"], b["w"]), what + ": flat_w"
        assert torch.equal(a["acc"], b["acc"]), what + ": acc"
        if a["v"] is not None:
            assert torch.equal(a["v"], b["v"]), what + ": v"
        assert set(a["pk"]) == set(b["pk"])
        for k in a["pk"]:
            assert torch.equal(a["pk"][k].view(torch.int16), b["pk"][k].view(torch.int16)), "%s: packed %s" % (what, k)

    def clipped_step_equals_plain(self, max_norm, like=None):
        """the clipping net's step at max_norm against the twin's plain step with the scale read back as gscale; returns the scale"""
        net, twin, n = self.net, self.twin, self.n
        net.clip_grad_norm = max_norm
        self.restore(net, like)
        before = self.snapshot(net)
        self.step(net)
        st = net.clip_stats()
        norm, scale = clip_scale(f32(st["sumsq"]), max_norm)
        assert f32(st["norm"]) == norm and f32(st["scale"]) == scale
        assert abs(st["norm"] / self.norm64 - 1.0) <= 29 * 2.0 ** -24   # (the bound of test_norm_of_random_values_..., a fortiori)
        self.restore(twin, like)
        self.step(twin, gscale=st["scale"])
        got, ref = self.snapshot(net), self.snapshot(twin)
        self.assert_same(got, ref, "max_norm %g" % max_norm)
        assert not torch.equal(got["w"][:n], before["w"][:n])
        # the dead level-(L-1) dilated pair behind n_live is never stepped
        assert torch.equal(got["w"][n:], before["w"][n:]) and torch.equal(got["acc"][n:], before["acc"][n:])
        assert (net.global_step, net.beta1_power, net.beta2_power) == (twin.global_step, twin.beta1_power, twin.beta2_power)
        return st


@pytest.mark.parametrize("optimizer", ["momentum", "adam"])
@pytest.mark.parametrize("L,root,dilated,P", [(3, 16, True, 20), (2, 16, False, 20)])
def test_clipped_step_equals_plain_step_with_the_scale(L, root, dilated, P, optimizer):
    """max_norm at half the gradient's float64 norm: the step is clipped (scale ~ 0.5) and equals, bit for bit in w, the slots and every
    packed buffer, the existing step with gscale = the scale read back. At twice the norm the scale is 1.0 and the bits are the default
    step's."""
    p = Pair(L, root, dilated, P, optimizer)
    st = p.clipped_step_equals_plain(0.5 * p.norm64)
    assert st["last_clipped"] and not st["last_skipped"] and abs(st["scale"] - 0.5) < 1e-5
    assert (st["steps"], st["clipped"], st["skipped"]) == (1, 1, 0)
    half = Pair.snapshot(p.net)
    st = p.clipped_step_equals_plain(2.0 * p.norm64)
    assert st["scale"] == 1.0 and not st["last_clipped"] and (st["steps"], st["clipped"], st["skipped"]) == (2, 1, 0)
    assert not torch.equal(half["w"], p.net.flat_w)   # (the clipped step was a different step)
    p.restore(p.twin)
    p.step(p.twin)                                    # the default step: gscale 1.0
    Pair.assert_same(Pair.snapshot(p.net), Pair.snapshot(p.twin), "unclipped against the default step")


@pytest.mark.parametrize("optimizer", ["momentum", "adam"])
def test_step_with_an_inf_in_the_gradient_is_skipped(optimizer):
    """an inf in one element of a conv kernel's gradient: apply_* leaves weights, slots and every packed buffer bit-identical, counts
    the step on the host (global_step, Adam's powers) and one skipped step on the device; the next step, with a finite gradient, is
    the oracle's clipped step from that state"""
    p = Pair(3, 16, True, 20, optimizer)
    net = p.net
    net.clip_grad_norm = 0.5 * p.norm64
    p.restore(net)
    net.g["conv_1/conv1/kernel"].view(-1)[7] = float("inf")
    before = Pair.snapshot(net)
    gs = net.global_step
    p.step(net)
    Pair.assert_same(Pair.snapshot(net), before, "skipped step")
    st = net.clip_stats()
    assert (st["steps"], st["clipped"], st["skipped"]) == (1, 0, 1) and st["last_skipped"] and st["scale"] == 0.0
    assert net.global_step == gs + 1
    if optimizer == "adam":
        assert (net.beta1_power, net.beta2_power) == (_power(0.9, 7), _power(0.999, 7))
    st = p.clipped_step_equals_plain(0.5 * p.norm64, like=(net.global_step, net.beta1_power, net.beta2_power))
    assert (st["steps"], st["clipped"], st["skipped"]) == (2, 1, 1) and not st["last_skipped"] and st["last_clipped"]


# ------------------------------------------------------------------------------------------- 6. the default step
@pytest.mark.parametrize("optimizer", ["momentum", "adam"])
def test_default_step_is_unchanged_and_a_huge_bound_only_measures(optimizer, monkeypatch):
    nets = [UNet(2, 16, False, 2, 20, seed=29, training=True, optimizer=optimizer, **kw) for kw in ({}, {"clip_grad_norm": 1e30})]
    plain, guard = nets
    assert plain.clip_grad_norm is None and plain.clip_state is None and plain._clip_ws is None and plain.clip_stats() is None
    assert guard.clip_state is not None and guard.clip_state.numel() * 4 == lib().rsu_clip_state_bytes()
    gen = torch.Generator(device="cpu").manual_seed(2)
    for _ in range(3):
        x = torch.rand((2, plain.S, plain.S, 3), generator=gen)
        y = (torch.rand((2, 20, 20), generator=gen) < 0.3).to(torch.int64)
        for m in nets:
            m.x.copy_(x); m.labels.copy_(y)
            m.forward_device()
            m.backward_device(1.0 / 800)
            m.apply_adam(0.01) if optimizer == "adam" else m.apply_momentum(0.01, 0.9)
    torch.cuda.synchronize()
    assert torch.equal(plain.flat_w, guard.flat_w) and torch.equal(plain.flat_acc, guard.flat_acc)
    for k in plain.pk:
        assert torch.equal(plain.pk[k].view(torch.int16), guard.pk[k].view(torch.int16)), k
    st = guard.clip_stats()
    assert (st["steps"], st["clipped"], st["skipped"]) == (3, 0, 0) and st["scale"] == 1.0 and st["norm"] > 0
    # the _clip entry points refuse a null state before anything is launched
    tab, w0 = guard._update_table, guard.flat_w.clone()
    assert lib().rsu_update_table_run_clip(tab[0].data_ptr(), tab[1], tab[2], 0.01, 0.9, 1.0, None, _stream()) == -22
    assert lib().rsu_update_table_run_adam_clip(tab[0].data_ptr(), tab[1], tab[2], 1e-3, 0.9, 0.999, 1e-8, 1.0, None, _stream()) == -22
    torch.cuda.synchronize()
    assert torch.equal(guard.flat_w, w0)
    # and the unfused developer path has no clipped variant
    monkeypatch.setenv("RSU_FUSED_UPDATE", "0")
    gs = guard.global_step
    with pytest.raises(RsuError, match="RSU_FUSED_UPDATE"):
        guard.apply_adam(0.01) if optimizer == "adam" else guard.apply_momentum(0.01, 0.9)
    assert guard.global_step == gs
    for bad in (0.0, -1.0, float("nan"), float("inf"), "x"):
        with pytest.raises(RsuError):
            UNet(2, 16, False, 2, 20, clip_grad_norm=bad)


# ------------------------------------------------------------------------------------------- 7. model and command line
def test_cli_trains_with_clipping_and_logs_the_norm(tmp_path, capsys):
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
    logs = tmp_path / "logs"
    argv = ["--num_layers=2", "--root_size=16", "--patch_size=16", "--stride=16", "--batch_size=4", "--num_epoch=1", "--lr=0.001",
            "--optimizer=adam", "--clip_grad_norm=0.05", "--train_data_dir=%s" % tr, "--save_path=%s" % (tmp_path / "runs"),
            "--logdir=%s" % logs, "--rotation_angles=0,90", "--seed=5"]
    assert main(argv) == 0
    out = capsys.readouterr().out
    m = re.search(r"'clip': \{'steps': (\d+), 'clipped': (\d+), 'skipped': (\d+), 'norm': ([^,]+), 'scale': ([^,]+),", out)
    assert m, out[-2000:]
    steps, clipped, skipped = int(m.group(1)), int(m.group(2)), int(m.group(3))
    runs = os.listdir(logs)
    assert len(runs) == 1
    events = [json.loads(line) for line in open(logs / runs[0] / "events.jsonl")]
    norms = [e for e in events if e["tag"] == "grad_norm"]
    losses = [e for e in events if e["tag"] == "loss"]
    assert steps > 0 and len(norms) == steps == len(losses)
    assert [e["step"] for e in norms] == [e["step"] for e in losses] == list(range(1, steps + 1))
    assert all(np.isfinite(e["value"]) and e["value"] > 0 for e in norms)
    assert skipped == 0 and clipped == sum(e["value"] > float(f32(0.05)) for e in norms)
    assert float(m.group(4)) == norms[-1]["value"]
