#!/usr/bin/env python3
"""Developer tool (GPU box): what --ema_decay costs.

  bench_ema.py pass
      rsu_ema_step alone at config 2's n_live: us per call (median of 30) and GB/s at 12 B per weight, and in the same process
      rsu_grad_norm (the figure tools/bench_clip.py norm reports, 4 B per weight) -- both to be read against the copy and read-only rates
      of profiles/*/hbm_rates.txt.
  bench_ema.py step --tree PARENT [--reps N] [--optimizer momentum|adam]
      the config-2 training step under three arms, alternating fresh processes on one box (the pattern of tools/clip_ab.sh): the
      parent commit's checkout PARENT (built, with its own library), this tree with the flag off, this tree with --ema_decay=0.999.
      Every process runs under its own time limit and the series stops at the first one that fails. The spread of the parent arm's
      runs is the noise the other two are read against; the summary at the end says whether the flag-off arm stays inside it.
  bench_ema.py arm [--tree DIR] [--ema D] [--optimizer momentum|adam] [--steps N]
      one arm of the above in this process: L = 5, root 64, 388 px, 4 patches; forward + backward + update on a fixed batch, dropout
      off as in bench.py; ms per step over N steps between two events after 10 warm-up steps. --tree DIR imports the package from
      another checkout (it needs --ema 0: the keyword does not exist in the parent).
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
ap.add_argument("mode", choices=["pass", "step", "arm"])
ap.add_argument("--tree", default=None)
ap.add_argument("--ema", type=float, default=0.0)
ap.add_argument("--optimizer", default="momentum")
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--reps", type=int, default=4)
a = ap.parse_args()

if a.mode == "step":
    if not a.tree:
        sys.exit("step needs --tree PARENT (a built checkout of the parent commit)")
    arms = [("parent", ["--tree", a.tree, "--ema", "0"]), ("off", ["--ema", "0"]), ("on", ["--ema", "0.999"])]
    ms = {k: [] for k, _ in arms}
    for rep in range(a.reps):
        for name, extra in arms:
            cmd = ["timeout", "-k", "10", "150", sys.executable, os.path.abspath(__file__), "arm", "--optimizer", a.optimizer,
                   "--steps", str(a.steps)] + extra
            r = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            m = re.search(r": ([0-9.]+) ms/step", r.stdout)
            if r.returncode != 0 or not m:
                sys.exit("arm %s failed (exit status %d): the series stops here" % (name, r.returncode))
            ms[name].append(float(m.group(1)))
    med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
    mean = {k: sum(v) / len(v) for k, v in ms.items()}
    spread = max(ms["parent"]) - min(ms["parent"])
    for k, _ in arms:
        print("%-6s ms/step: %s | mean %.4f median %.4f min %.4f max %.4f" % (k, " ".join("%.4f" % v for v in ms[k]), mean[k], med[k],
                                                                              min(ms[k]), max(ms[k])))
    d_off, d_on = mean["off"] - mean["parent"], mean["on"] - mean["off"]
    print("parent arm's run-to-run spread (max - min): %.4f ms" % spread)
    print("flag off - parent (means): %+.4f ms (%+.2f %%): %s the parent's spread" % (d_off, 100 * d_off / mean["parent"],
                                                                                     "inside" if abs(d_off) <= spread else "OUTSIDE"))
    print("flag on - flag off (means): %+.4f ms (%+.2f %%) per step" % (d_on, 100 * d_on / mean["off"]))
    sys.exit(0)

sys.path.insert(0, os.path.abspath(a.tree or HERE))

import torch  # noqa: E402
from road_segmentation_unet_amd import _lib  # noqa: E402
from road_segmentation_unet_amd.unet import UNet  # noqa: E402

L, ROOT_SIZE, DIL, B, P = 5, 64, False, 4, 388
sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]


def median_us(fn, reps=30):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record(); fn(); e.record(); e.synchronize()
        ts.append(s.elapsed_time(e) * 1e3)
    return sorted(ts)[len(ts) // 2]


def net(**kw):
    m = UNet(L, ROOT_SIZE, DIL, B, P, training=True, optimizer=a.optimizer, **kw)
    gen = torch.Generator(device="cpu").manual_seed(0)
    m.x.copy_(torch.rand((B, m.S, m.S, 3), generator=gen))
    m.labels.copy_((torch.rand((B, P, P), generator=gen) < 0.2).to(torch.int64))
    return m


if a.mode == "arm":
    m = net(**({"ema_decay": a.ema} if a.ema > 0 else {}))
    m.ensure_tuned()
    inv = 1.0 / (B * P * P)

    def step():
        m.forward_device()
        m.backward_device(inv)
        m.apply_adam(1e-4) if a.optimizer == "adam" else m.apply_momentum(0.001, 0.9)
    for _ in range(10):
        step()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(a.steps):
        step()
    e.record(); e.synchronize()
    ms = s.elapsed_time(e) / a.steps
    print("step %s ema %g tree %s lib %s: %.4f ms/step = %.1f patches/s (%d steps)"
          % (a.optimizer, a.ema, os.path.basename(os.path.abspath(a.tree or HERE)), sha, ms, B / ms * 1e3, a.steps))
else:
    m = net(ema_decay=0.999, clip_grad_norm=1e30)
    m.flat_g.normal_(0, 1e-3)
    n = m.n_live
    print("lib %s, %d live weights (%.1f MB per array), device %s" % (sha, n, n * 4 / 1e6, torch.cuda.get_device_name(0)))
    m.global_step = 100000   # (past the warm-up: the decay is 0.999)
    us_e = median_us(m._ema_step)
    us_n = median_us(m._grad_norm)
    gb_e, gb_n = n * 12 / us_e / 1e3, n * 4 / us_n / 1e3
    print("rsu_ema_step: %.1f us (median of 30) = %.0f GB/s at 12 B per weight" % (us_e, gb_e))
    print("rsu_grad_norm (both launches): %.1f us (median of 30) = %.0f GB/s at 4 B per weight" % (us_n, gb_n))
    print("rsu_ema_step moves bytes at %.2f x the rate of rsu_grad_norm; fused into the update pass it would move 8 of these 12 B: "
          "about %.1f us of the %.1f to recover" % (gb_e / gb_n, us_e / 3.0, us_e))
