#!/usr/bin/env python3
"""Developer tool (GPU box): what --focal_gamma costs.

  bench_focal.py heads
      the heads alone at config 2's head shape (npix = 4 x 388 x 388, C = 64), in one process, the arms of a pair alternated call by
      call: rsu_head_fwd_bwd_w against rsu_head_fwd_bwd_focal at gamma = 2; rsu_head_dice_sums + rsu_head_fwd_bwd_dice against
      rsu_head_dice_sums + rsu_head_fwd_bwd_focal with the Dice term; rsu_head_eval against rsu_head_eval_focal. us per call (median of
      30 rounds, with min and max: an arm's own run-to-run spread) and GB/s of activations read and gradients written.
  bench_focal.py step --lib PARENT_LIBRARY [--reps N]
      the DEFAULT config-2 training step (no flag of this change set) with this tree's library against the parent commit's library
      (built as `make -C road_segmentation_unet_amd/csrc VARIANT=parent` in a checkout of the parent, loaded through RSU_LIB_PATH),
      alternating fresh processes on one box (the pattern of tools/bench_decay.py; the order of the arms rotates from round to round). Every process runs under its own time limit and the
      series stops at the first one that fails. Medians per arm; the spread of the parent arm's runs is the noise the difference is read
      against.
  bench_focal.py arm [--gamma G] [--steps N]
      one arm of the above in this process: L = 5, root 64, 388 px, 4 patches; forward + backward + update on a fixed batch, dropout off
      as in bench.py; ms per step over N steps between two events after 10 warm-up steps. The library is RSU_LIB_PATH's or the tree's;
      --parent-lib: that library is the parent commit's, which has no entry of rsu_loss.h -- the table is left unbound (the default
      step calls none of them).
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
ap.add_argument("mode_", metavar="mode", choices=["heads", "step", "arm"])
ap.add_argument("--lib", default=None)
ap.add_argument("--gamma", type=float, default=0.0)
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--parent-lib", action="store_true")
a = ap.parse_args()


def median(v):
    return sorted(v)[len(v) // 2]


if a.mode_ == "step":
    if not a.lib or not os.path.exists(a.lib):
        sys.exit("step needs --lib: the parent commit's library")
    arms = [("parent", {"RSU_LIB_PATH": os.path.abspath(a.lib)}, ["--parent-lib"]), ("default", {}, []), ("focal", {}, ["--gamma", "2"])]
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
    d = med["focal"] - med["default"]
    print("--focal_gamma=2 - default (medians): %+.4f ms (%+.2f %%) per step (the weighted-family head in place of the pinned one)"
          % (d, 100 * d / med["default"]))
    sys.exit(0)

sys.path.insert(0, HERE)

import torch  # noqa: E402
from road_segmentation_unet_amd import _lib  # noqa: E402
from road_segmentation_unet_amd.unet import UNet, _ptr  # noqa: E402

if a.parent_lib:
    _lib.SIGNATURES_LOSS.clear()
L, ROOT_SIZE, DIL, B, P = 5, 64, False, 4, 388
sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]

if a.mode_ == "arm":
    m = UNet(L, ROOT_SIZE, DIL, B, P, training=True, **({"focal_gamma": a.gamma} if a.gamma > 0 else {}))
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
    print("step gamma %g lib %s: %.4f ms/step = %.1f patches/s (%d steps)" % (a.gamma, sha, ms, B / ms * 1e3, a.steps))
    sys.exit(0)

# ---- heads
print("lib %s, device %s" % (sha, torch.cuda.get_device_name(0)))
C, NPIX, GAMMA, LAM, SMOOTH = ROOT_SIZE, B * P * P, 2.0, 0.7, 1.0
dev = "cuda:0"
gen = torch.Generator(device="cpu").manual_seed(1)
act = torch.relu(torch.randn((NPIX, C), generator=gen)).to(dev).to(torch.bfloat16)
w, b = (0.3 * torch.randn((C, 2), generator=gen)).to(dev), (0.1 * torch.randn(2, generator=gen)).to(dev)
lab = (torch.rand(NPIX, generator=gen) < 0.2).to(torch.int64)
lab[torch.rand(NPIX, generator=gen) < 0.05] = -1
lab = lab.to(dev)
pw = (0.25 + torch.rand(NPIX, generator=gen)).to(dev)
cw = torch.tensor([0.6, 2.5], device=dev)
z = lambda *s, dtype=torch.float32: torch.zeros(s, dtype=dtype, device=dev)  # noqa: E731
prob, dact, dw, db, loss, wsum, dsums = z(NPIX), z(NPIX, C, dtype=torch.bfloat16), z(C, 2), z(2), z(1), z(1), z(3)
esums, hist = z(5), z(2, 256, dtype=torch.int64)
lib = _lib.lib()
ws = z(max(lib.rsu_head_dice_ws_floats(NPIX, C), lib.rsu_head_eval_ws_floats(NPIX, C)))
st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
head = (_ptr(act), _ptr(w), _ptr(b), _ptr(lab))
tail = lambda: (_ptr(prob), _ptr(loss), _ptr(wsum), _ptr(dact), _ptr(dw), _ptr(db), _ptr(ws), NPIX, C, 1.0 / NPIX, st())  # noqa: E731


def sums_pass():
    _lib.call("rsu_head_dice_sums", *head, _ptr(pw), _ptr(prob), _ptr(dsums), _ptr(ws), NPIX, C, st())


def dice():
    sums_pass()
    _lib.call("rsu_head_fwd_bwd_dice", *head, _ptr(cw), _ptr(pw), _ptr(dsums), LAM, SMOOTH, *tail())


def focal_dice():
    sums_pass()
    _lib.call("rsu_head_fwd_bwd_focal", *head, _ptr(cw), _ptr(pw), GAMMA, _ptr(dsums), LAM, SMOOTH, *tail())


pairs = [
    ("training head", 2 * NPIX * C * 2, [
        ("weighted", lambda: _lib.call("rsu_head_fwd_bwd_w", *head, _ptr(cw), _ptr(pw), *tail())),
        ("focal", lambda: _lib.call("rsu_head_fwd_bwd_focal", *head, _ptr(cw), _ptr(pw), GAMMA, None, 0.0, 0.0, *tail()))]),
    ("training head with the Dice term (two launches)", 3 * NPIX * C * 2, [("dice", dice), ("focal+dice", focal_dice)]),
    ("evaluation head", NPIX * C * 2, [
        ("eval", lambda: _lib.call("rsu_head_eval", *head, _ptr(cw), _ptr(pw), _ptr(prob), _ptr(esums), _ptr(hist), _ptr(ws), NPIX, C, st())),
        ("eval focal", lambda: _lib.call("rsu_head_eval_focal", *head, _ptr(cw), _ptr(pw), GAMMA, _ptr(prob), _ptr(esums), _ptr(hist), _ptr(ws),
                                         NPIX, C, st()))]),
]
print("npix = %d x %d x %d = %d, C = %d, gamma = %g, class weights, a weight map, 5 %% ignored labels" % (B, P, P, NPIX, C, GAMMA))
for title, nbytes, arms in pairs:
    for _ in range(5):
        for _name, fn in arms:
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k, _ in arms}
    for _ in range(30):
        for name, fn in arms:
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record(); fn(); e.record(); e.synchronize()
            us[name].append(s.elapsed_time(e) * 1e3)
    base = arms[0][0]
    print("%s (%.1f MB of activations and their gradients per call):" % (title, nbytes / 1e6))
    for name, _fn in arms:
        u = median(us[name])
        print("  %-11s %.1f us (median of 30, min %.1f max %.1f) = %.0f GB/s; against %s %+.1f us (%+.2f %%)"
              % (name, u, min(us[name]), max(us[name]), nbytes / u / 1e3, base, u - median(us[base]),
                 100 * (u - median(us[base])) / median(us[base])))
    spread = max(us[base]) - min(us[base])
    d = median(us[arms[1][0]]) - median(us[base])
    print("  the %s arm's own spread (max - min) %.1f us: the focal arm's median lies %s it (%+.1f us)"
          % (base, spread, "inside" if abs(d) <= spread else "OUTSIDE", d))
