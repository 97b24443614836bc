#!/usr/bin/env python3
"""Developer tool (GPU box): what the clDice term (--cldice_weight, include/rsu_cldice.h) costs.

  bench_cldice.py kernels
      rsu_cldice_fwd and rsu_cldice_bwd alone at config 2's head shape (B = 4, 388 x 388) for iters 3, 10 and 16, against the torch
      restatement of the same term (max_pool2d plus autograd, float32) on the same device and inputs, in one process, the arms
      alternated call by call: us per call (median of 20 rounds, with min and max: an arm's own run-to-run spread). Then the whole head
      sequence with the term on (pass A, the zeroing, forward, backward, aux head) against the Dice head's two launches.
  bench_cldice.py step --lib PARENT_LIBRARY [--reps N]
      the DEFAULT config-2 training step (no flag of this change set) with this tree's library against the parent commit's library
      (built as `make -C road_segmentation_unet_amd/csrc VARIANT=parent` in a checkout of the parent, loaded through RSU_LIB_PATH),
      and the step with --cldice_weight=1 --cldice_iters=10, alternating fresh processes on one box (the pattern of
      tools/bench_focal.py; the order of the arms rotates from round to round). Every process runs under its own time limit and the
      series stops at the first one that fails. Medians per arm; the spread of the parent arm's runs is the noise the difference is read
      against.
  bench_cldice.py arm [--cldice W] [--iters K] [--steps N]
      one arm of the above in this process: L = 5, root 64, 388 px, 4 patches; forward + backward + update on a fixed batch, dropout off
      as in bench.py; ms per step over N steps between two events after 10 warm-up steps. --parent-lib: the library is the parent
      commit's, which has no entry of rsu_cldice.h -- the table is left unbound (the default step calls none of them).
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
ap.add_argument("mode_", metavar="mode", choices=["kernels", "step", "arm"])
ap.add_argument("--lib", default=None)
ap.add_argument("--cldice", type=float, default=0.0)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--parent-lib", action="store_true")
a = ap.parse_args()


def median(v):
    return sorted(v)[len(v) // 2]


if a.mode_ == "step":
    if not a.lib or not os.path.exists(a.lib):
        sys.exit("step needs --lib: the parent commit's library")
    arms = [("parent", {"RSU_LIB_PATH": os.path.abspath(a.lib)}, ["--parent-lib"]), ("default", {}, []),
            ("cldice", {}, ["--cldice", "1", "--iters", "10"])]
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
    d = med["cldice"] - med["default"]
    print("--cldice_weight=1 --cldice_iters=10 - default (medians): %+.4f ms (%+.2f %%) per step" % (d, 100 * d / med["default"]))
    sys.exit(0)

sys.path.insert(0, HERE)

import torch  # noqa: E402
import torch.nn.functional as Fn  # noqa: E402
from road_segmentation_unet_amd import _lib  # noqa: E402
from road_segmentation_unet_amd.unet import UNet, _ptr  # noqa: E402

if a.parent_lib:
    _lib.SIGNATURES_CLDICE.clear()
L, ROOT_SIZE, DIL, B, P = 5, 64, False, 4, 388
sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]

if a.mode_ == "arm":
    m = UNet(L, ROOT_SIZE, DIL, B, P, training=True, **({"cldice_weight": a.cldice, "cldice_iters": a.iters} if a.cldice > 0 else {}))
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
    print("step cldice %g iters %d lib %s: %.4f ms/step = %.1f patches/s (%d steps)" % (a.cldice, a.iters, sha, ms, B / ms * 1e3, a.steps))
    sys.exit(0)

# ---- kernels
print("lib %s, device %s" % (sha, torch.cuda.get_device_name(0)))
dev = "cuda:0"
C, NPIX, SCALE, SMOOTH, LAM = ROOT_SIZE, B * P * P, 1.0, 1.0, 0.7
gen = torch.Generator(device="cpu").manual_seed(1)
# a smooth road-like map (blurred noise through a sigmoid) and its thresholded labels, 5 % of them ignored
noise = torch.randn((B, 1, P, P), generator=gen)
for _ in range(6):
    noise = Fn.avg_pool2d(noise, 5, 1, 2)
prob = torch.sigmoid(noise[:, 0] / noise.std() * 3.0).contiguous()
lab = (prob > 0.6).to(torch.int64)
lab[torch.rand((B, P, P), generator=gen) < 0.05] = -1
prob, lab = prob.to(dev), lab.to(dev)
z = lambda *s, dtype=torch.float32: torch.zeros(s, dtype=dtype, device=dev)  # noqa: E731
skel_p, skel_y, gprob, sums = z(B, P, P), z(B, P, P), z(B, P, P), z(4)
lib = _lib.lib()
cws = z(lib.rsu_cldice_ws_floats(B, P, P, 16))
st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731


def fwd(k):
    sums.zero_()
    _lib.call("rsu_cldice_fwd", _ptr(prob), _ptr(lab), k, _ptr(skel_p), _ptr(skel_y), _ptr(sums), _ptr(cws), B, P, P, st())


def bwd(k):
    _lib.call("rsu_cldice_bwd", _ptr(prob), _ptr(lab), _ptr(skel_p), _ptr(skel_y), _ptr(sums), k, SCALE, SMOOTH, _ptr(gprob), _ptr(cws), B, P, P, st())


def t_erode(x):
    return torch.minimum(-Fn.max_pool2d(-x, (3, 1), 1, (1, 0)), -Fn.max_pool2d(-x, (1, 3), 1, (0, 1)))


def t_skel(x, k):
    x = x[:, None]
    skel = torch.relu(x - Fn.max_pool2d(t_erode(x), 3, 1, 1))
    for _ in range(k):
        x = t_erode(x)
        d = torch.relu(x - Fn.max_pool2d(t_erode(x), 3, 1, 1))
        skel = skel + torch.relu(d - skel * d)
    return skel[:, 0]


mf, yf = ((lab == 0) | (lab == 1)).float(), (lab == 1).float()
state = {}


def t_fwd(k):
    p = prob.detach().clone().requires_grad_(True)
    sp, sy = t_skel(p, k), t_skel(yf, k)
    Tp = ((mf * sp * yf).sum() + SMOOTH) / ((mf * sp).sum() + SMOOTH)
    Ts = ((mf * sy * p).sum() + SMOOTH) / ((mf * sy).sum() + SMOOTH)
    state["p"], state["term"] = p, SCALE * (1.0 - 2.0 * Tp * Ts / (Tp + Ts))


def t_bwd(k):
    state["term"].backward()


def timed(arms, rounds=20, pre=None):
    for _ in range(3):
        for _n, fn in arms:
            if pre:
                pre()
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k, _ in arms}
    for _ in range(rounds):
        for name, fn in arms:
            if pre:
                pre()
                torch.cuda.synchronize()
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(); fn(); e.record(); e.synchronize()
            us[name].append(s.elapsed_time(e) * 1e3)
    return us


print("B x H x W = %d x %d x %d, 5 %% ignored labels; us per call, median of 20 (min .. max)" % (B, P, P))
for k in (3, 10, 16):
    f = timed([("fused fwd", lambda: fwd(k)), ("torch fwd", lambda: t_fwd(k))])
    # the backward arms need a forward in front of each call (torch frees its graph; the fused one reads the forward's workspace)
    fwd(k)
    bk = timed([("fused bwd", lambda: bwd(k))])
    tb = timed([("torch bwd", lambda: t_bwd(k))], pre=lambda: t_fwd(k))
    tg = state["p"].grad * mf      # (an ignored pixel is a constant of the fused term)
    hu_err = float((gprob - tg).abs().max()) / max(1e-30, float(tg.abs().max()))
    for name, u in list(f.items()) + list(bk.items()) + list(tb.items()):
        print("  iters %2d %-10s %9.1f us (%.1f .. %.1f)" % (k, name, median(u), min(u), max(u)))
    print("  iters %2d fused pair %.1f us, torch pair %.1f us: x %.1f; max |gprob - autograd| / max |autograd| %.2e (ties are routed differently)"
          % (k, median(f["fused fwd"]) + median(bk["fused bwd"]), median(f["torch fwd"]) + median(tb["torch bwd"]),
             (median(f["torch fwd"]) + median(tb["torch bwd"])) / (median(f["fused fwd"]) + median(bk["fused bwd"])), hu_err))

# ---- the whole head sequence with the term on, against the Dice head's two launches
act = torch.relu(torch.randn((NPIX, C), generator=gen)).to(dev).to(torch.bfloat16)
w, b = (0.3 * torch.randn((C, 2), generator=gen)).to(dev), (0.1 * torch.randn(2, generator=gen)).to(dev)
labf = lab.reshape(-1)
hprob, dact, dw, db, loss, wsum, dsums = z(B, P, P), z(NPIX, C, dtype=torch.bfloat16), z(C, 2), z(2), z(1), z(1), z(3)
ws = z(lib.rsu_head_dice_ws_floats(NPIX, C))
head = (_ptr(act), _ptr(w), _ptr(b), _ptr(labf))
tail = lambda: (_ptr(hprob), _ptr(loss), _ptr(wsum), _ptr(dact), _ptr(dw), _ptr(db), _ptr(ws), NPIX, C, 1.0 / NPIX)  # noqa: E731


def dice():
    _lib.call("rsu_head_dice_sums", *head, None, _ptr(hprob), _ptr(dsums), _ptr(ws), NPIX, C, st())
    _lib.call("rsu_head_fwd_bwd_dice", *head, None, None, _ptr(dsums), LAM, SMOOTH, *tail(), st())


def cldice_seq(k, with_dice):
    if with_dice:
        _lib.call("rsu_head_dice_sums", *head, None, _ptr(hprob), _ptr(dsums), _ptr(ws), NPIX, C, st())
    else:
        _lib.call("rsu_head_fwd", _ptr(act), _ptr(w), _ptr(b), _ptr(hprob), None, NPIX, C, st())
    sums.zero_()
    _lib.call("rsu_cldice_fwd", _ptr(hprob), _ptr(lab), k, _ptr(skel_p), _ptr(skel_y), _ptr(sums), _ptr(cws), B, P, P, st())
    _lib.call("rsu_cldice_bwd", _ptr(hprob), _ptr(lab), _ptr(skel_p), _ptr(skel_y), _ptr(sums), k, SCALE, SMOOTH, _ptr(gprob), _ptr(cws), B, P, P, st())
    _lib.call("rsu_head_fwd_bwd_aux", *head, None, None, 0.0, _ptr(dsums) if with_dice else None, LAM, SMOOTH, *tail(), _ptr(gprob), st())


us = timed([("dice head", dice), ("clDice k=10", lambda: cldice_seq(10, False)), ("clDice k=10 + dice", lambda: cldice_seq(10, True)),
            ("clDice k=16", lambda: cldice_seq(16, False))])
print("the head sequence at npix = %d, C = %d (the prob map of a random head: noise, the skeletons' worst case for ties):" % (NPIX, C))
for name, u in us.items():
    print("  %-20s %9.1f us (%.1f .. %.1f); against the dice head %+.1f us" % (name, median(u), min(u), max(u), median(u) - median(us["dice head"])))
