#!/usr/bin/env python3
"""Developer tool (GPU box): what the Lovasz term (--lovasz_weight, include/rsu_lovasz.h) costs.

  bench_lovasz.py kernels
      rsu_lovasz_fwd_bwd and rsu_lovasz_fwd alone at config 2's head shape (B = 4, 388 x 388) against the float32 torch statement of
      the same term (torch.sort along each image, gather, cumsum, autograd) on the same device and inputs, in one process, the arms
      alternated call by call: us per call (median of 20 rounds, with min and max: an arm's own run-to-run spread).
  bench_lovasz.py split [--calls N]
      N calls of rsu_lovasz_fwd_bwd and nothing else: the process to put behind `rocprofv3 --kernel-trace --stats --` for the
      per-kernel split (k_lv_local<true> builds and sorts the tiles, k_lv_global<R> and k_lv_local<false> merge, k_lv_grad, k_lv_final).
  bench_lovasz.py step --lib PARENT_LIBRARY [--reps N]
      the DEFAULT config-2 training step (no flag of this change set) with this tree's library against the parent commit's library
      (built as `make -C road_segmentation_unet_amd/csrc VARIANT=parent` in a checkout of the parent, loaded through RSU_LIB_PATH),
      and the step with --lovasz_weight=1, alternating fresh processes on one box (the pattern of tools/bench_cldice.py; the order of
      the arms rotates from round to round). Every process runs under its own time limit and the series stops at the first one that
      fails. Medians per arm; the spread of the parent arm's runs is the noise the difference is read against.
  bench_lovasz.py arm [--lovasz W] [--steps N]
      one arm of the above in this process: L = 5, root 64, 388 px, 4 patches; forward + backward + update on a fixed batch, dropout off
      as in bench.py; ms per step over N steps between two events after 10 warm-up steps. --parent-lib: the library is the parent
      commit's, which has no entry of rsu_lovasz.h -- the table is left unbound (the default step calls none of them).
The record goes to standard output: keep it under profiles/rNN/.
"""
import argparse
import hashlib
import os
import re
import subprocess
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("mode_", metavar="mode", choices=["kernels", "split", "step", "arm"])
ap.add_argument("--lib", default=None)
ap.add_argument("--lovasz", type=float, default=0.0)
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--parent-lib", action="store_true")
a = ap.parse_args()


def median(v):
    return sorted(v)[len(v) // 2]


if a.mode_ == "step":
    if not a.lib or not os.path.exists(a.lib):
        sys.exit("step needs --lib: the parent commit's library")
    arms = [("parent", {"RSU_LIB_PATH": os.path.abspath(a.lib)}, ["--parent-lib"]), ("default", {}, []), ("lovasz", {}, ["--lovasz", "1"])]
    ms = {k: [] for k, _, _ in arms}
    for rep in range(a.reps):
        for name, env, extra in arms[rep % len(arms):] + arms[:rep % len(arms)]:   # (no arm is always the first of its round)
            cmd = ["timeout", "-k", "10", "150", sys.executable, os.path.abspath(__file__), "arm", "--steps", str(a.steps)] + extra
            e = {k: v for k, v in os.environ.items() if k != "RSU_LIB_PATH"}
            e.update(env)
            r = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True, env=e)
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            m = re.search(r": ([0-9.]+) ms/step", r.stdout)
            if r.returncode != 0 or not m:
                sys.exit("arm %s failed (exit status %d): the series stops here" % (name, r.returncode))
            ms[name].append(float(m.group(1)))
    med = {k: median(v) for k, v in ms.items()}
    for k, _, _ in arms:
        print("%-8s ms/step: %s | median %.4f min %.4f max %.4f" % (k, " ".join("%.4f" % v for v in ms[k]), med[k], min(ms[k]), max(ms[k])))
    spread = max(ms["parent"]) - min(ms["parent"])
    print("the parent arm's run-to-run spread (max - min): %.4f ms" % spread)
    d = med["default"] - med["parent"]
    print("default step, this library - parent's (medians): %+.4f ms (%+.2f %%): %s the parent's spread"
          % (d, 100 * d / med["parent"], "inside" if abs(d) <= spread else "OUTSIDE"))
    d = med["lovasz"] - med["default"]
    print("--lovasz_weight=1 - default (medians): %+.4f ms (%+.2f %%) per step" % (d, 100 * d / med["default"]))
    sys.exit(0)

sys.path.insert(0, HERE)

import torch  # noqa: E402
import torch.nn.functional as Fn  # noqa: E402
from road_segmentation_unet_amd import _lib  # noqa: E402
from road_segmentation_unet_amd.unet import UNet, _ptr  # noqa: E402

if a.parent_lib:
    _lib.SIGNATURES_LOVASZ.clear()
L, ROOT_SIZE, DIL, B, P = 5, 64, False, 4, 388
sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]

if a.mode_ == "arm":
    m = UNet(L, ROOT_SIZE, DIL, B, P, training=True, **({"lovasz_weight": a.lovasz} if a.lovasz > 0 else {}))
    gen = torch.Generator(device="cpu").manual_seed(0)
    m.x.copy_(torch.rand((B, m.S, m.S, 3), generator=gen))
    m.labels.copy_((torch.rand((B, P, P), generator=gen) < 0.2).to(torch.int64))
    m.ensure_tuned()
    inv = 1.0 / (B * P * P)

    def step():
        m.forward_device()
        m.backward_device(inv)
        m.apply_momentum(0.001, 0.9)
    for _ in range(10):
        step()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(a.steps):
        step()
    e.record(); e.synchronize()
    ms = s.elapsed_time(e) / a.steps
    print("step lovasz %g lib %s: %.4f ms/step = %.1f patches/s (%d steps)" % (a.lovasz, sha, ms, B / ms * 1e3, a.steps))
    sys.exit(0)

# ---- kernels / split
print("lib %s, device %s" % (sha, torch.cuda.get_device_name(0)))
dev = "cuda:0"
SCALE = 1.0
gen = torch.Generator(device="cpu").manual_seed(1)
# a smooth road-like map (blurred noise through a sigmoid) and its thresholded labels, 5 % of them ignored
noise = torch.randn((B, 1, P, P), generator=gen)
for _ in range(6):
    noise = Fn.avg_pool2d(noise, 5, 1, 2)
prob = torch.sigmoid(noise[:, 0] / noise.std() * 3.0).contiguous()
lab = (prob > 0.6).to(torch.int64)
lab[torch.rand((B, P, P), generator=gen) < 0.05] = -1
prob, lab = prob.to(dev), lab.to(dev)
lib = _lib.lib()
gprob = torch.zeros((B, P, P), dtype=torch.float32, device=dev)
loss = torch.zeros(2, dtype=torch.float32, device=dev)
ws = torch.zeros(lib.rsu_lovasz_ws_bytes(B, P, P) // 4, dtype=torch.int32, device=dev)
st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731


def fused():
    loss.zero_()
    _lib.call("rsu_lovasz_fwd_bwd", _ptr(prob), _ptr(lab), SCALE, 0, _ptr(gprob), _ptr(loss), _ptr(ws), B, P, P, st())


def fused_fwd():
    loss.zero_()
    _lib.call("rsu_lovasz_fwd", _ptr(prob), _ptr(lab), _ptr(loss), _ptr(ws), B, P, P, st())


if a.mode_ == "split":
    for _ in range(a.calls):
        fused()
    torch.cuda.synchronize()
    print("%d calls of rsu_lovasz_fwd_bwd at %d x %d x %d; loss_sum %s" % (a.calls, B, P, P, loss.tolist()))
    sys.exit(0)

mf, yf = ((lab == 0) | (lab == 1)).float().reshape(B, -1), (lab == 1).float().reshape(B, -1)
state = {}


def torch_arm():
    """the same term in float32 torch: the images as rows; ignored pixels sort last (error -1) and are masked out of every sum"""
    p = prob.detach().clone().requires_grad_(True)
    e = torch.where(mf > 0, (yf - p.reshape(B, -1)).abs(), torch.full_like(mf, -1.0))
    es, perm = torch.sort(e, dim=1, descending=True, stable=True)
    ys, msk = torch.gather(yf, 1, perm), torch.gather(mf, 1, perm)
    gts = ys.sum(1, keepdim=True)
    inter = gts - ys.cumsum(1)
    union = gts + ((1.0 - ys) * msk).cumsum(1)
    jac = 1.0 - inter / union.clamp_min(1.0)
    grad = torch.cat([jac[:, :1], jac[:, 1:] - jac[:, :-1]], 1)
    total = (torch.relu(es) * grad * msk).sum(1).mean() * SCALE
    total.backward()
    state["p"], state["total"] = p, total.detach()


def timed(arms, rounds=20):
    for _ in range(3):
        for _n, fn in arms:
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k, _ in arms}
    for _ in range(rounds):
        for name, fn in arms:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(); fn(); e.record(); e.synchronize()
            us[name].append(s.elapsed_time(e) * 1e3)
    return us


print("B x H x W = %d x %d x %d, 5 %% ignored labels; us per call, median of 20 (min .. max)" % (B, P, P))
us = timed([("fused fwd+bwd", fused), ("fused fwd", fused_fwd), ("torch fwd+bwd", torch_arm)])
for name, u in us.items():
    print("  %-14s %9.1f us (%.1f .. %.1f)" % (name, median(u), min(u), max(u)))
fused()
torch.cuda.synchronize()
tg = state["p"].grad
err = float((gprob - tg).abs().max()) / max(1e-30, float(tg.abs().max()))
fm, tm = median(us["fused fwd+bwd"]), median(us["torch fwd+bwd"])
print("  fused %.1f us, torch %.1f us: the %s arm is faster, x %.2f; loss fused %.7f torch %.7f; max |gprob - autograd| / max |autograd| %.2e"
      % (fm, tm, "fused" if fm < tm else "torch", max(fm, tm) / min(fm, tm), float(loss[0] / loss[1]) * SCALE, float(state["total"]), err))
