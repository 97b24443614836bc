#!/usr/bin/env python3
"""Developer tool (GPU box): what --accumulate_steps costs.

  bench_accum.py pass
      rsu_grad_accumulate alone at config 2's n_live, both variants: us per call (median of 30) and GB/s at 8 B per weight (assign:
      dst = src, dst is not read) and at 12 B per weight (dst += src), and in the same process rsu_ema_step, which moves the same
      12 B per weight -- all to be read against the copy and read-only rates of profiles/*/hbm_rates.txt.
  bench_accum.py step --tree PARENT [--reps N] [--optimizer momentum|adam]
      the config-2 training step under three arms, alternating fresh processes on one box (the pattern of tools/bench_ema.py): the
      parent commit's checkout PARENT (built, with its own library), this tree with the flag off, this tree with accumulate_steps=2
      at a micro-batch of 4 patches (an effective batch of 8: two forward + backward passes and one update per optimizer step).
      Every process runs under its own time limit and the series stops at the first one that fails. The spread of the parent arm's
      runs is the noise the flag-off arm is read against; the accumulating arm's optimizer step is read against TWICE the flag-off
      step, which takes one update per 4 patches where it takes one per 8.
  bench_accum.py arm [--tree DIR] [--accum K] [--optimizer momentum|adam] [--steps N]
      one arm of the above in this process: L = 5, root 64, 388 px, 4 patches per pass; K x (forward + backward [+ accumulate]) +
      update on a fixed batch, dropout off as in bench.py; ms per optimizer step over N steps between two events after 10 warm-up
      steps. --tree DIR imports the package from another checkout (it needs --accum 1: the keyword does not exist in the parent).
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
ap.add_argument("--accum", type=int, default=1)
ap.add_argument("--optimizer", default="momentum")
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--reps", type=int, default=4)
a = ap.parse_args()

if a.mode == "step":
    if not a.tree:
        sys.exit("step needs --tree PARENT (a built checkout of the parent commit)")
    arms = [("parent", ["--tree", a.tree, "--accum", "1"]), ("off", ["--accum", "1"]), ("on", ["--accum", "2"])]
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
    d_off, d_on = mean["off"] - mean["parent"], mean["on"] - 2 * mean["off"]
    print("parent arm's run-to-run spread (max - min): %.4f ms" % spread)
    print("flag off - parent (means): %+.4f ms (%+.2f %%): %s the parent's spread" % (d_off, 100 * d_off / mean["parent"],
                                                                                     "inside" if abs(d_off) <= spread else "OUTSIDE"))
    print("accumulate_steps=2, 8 patches per optimizer step: %.4f ms against 2 x flag off = %.4f ms: %+.4f ms (%+.2f %%) per optimizer step, "
          "%+.4f ms per micro-batch; %.1f against %.1f patches/s"
          % (mean["on"], 2 * mean["off"], d_on, 100 * d_on / (2 * mean["off"]), d_on / 2, 8 / mean["on"] * 1e3, 4 / mean["off"] * 1e3))
    sys.exit(0)

if a.tree and a.accum != 1:
    sys.exit("--tree imports another checkout, which may not know accumulate_steps: it needs --accum 1")
sys.path.insert(0, os.path.abspath(a.tree or HERE))

import torch  # noqa: E402
from road_segmentation_unet_amd import _lib  # noqa: E402
from road_segmentation_unet_amd._lib import call  # noqa: E402
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
    K = a.accum
    m = net(**({"accumulate_steps": K} if K > 1 else {}))
    m.ensure_tuned()
    inv = 1.0 / (K * B * P * P)

    def step():
        for _ in range(K):
            m.forward_device()
            m.backward_device(inv)
            if K > 1:
                m.accumulate_gradients()
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
    print("step %s accumulate_steps %d tree %s lib %s: %.4f ms/step = %.1f patches/s (%d optimizer steps of %d patches)"
          % (a.optimizer, K, os.path.basename(os.path.abspath(a.tree or HERE)), sha, ms, K * B / ms * 1e3, a.steps, K * B))
else:
    m = net(ema_decay=0.999, accumulate_steps=2)
    m.flat_g.normal_(0, 1e-3)
    n, st = m.n_live, m._stream
    print("lib %s, %d live weights (%.1f MB per array), device %s" % (sha, n, n * 4 / 1e6, torch.cuda.get_device_name(0)))
    m.global_step = 100000   # (past the warm-up: the decay is 0.999)
    g, gsum = m.flat_g.data_ptr(), m.flat_gsum.data_ptr()
    us_a = median_us(lambda: call("rsu_grad_accumulate", gsum, g, n, 1, st()))
    us_s = median_us(lambda: call("rsu_grad_accumulate", gsum, g, n, 0, st()))
    us_e = median_us(m._ema_step)
    print("rsu_grad_accumulate assign (gsum = g):  %.1f us (median of 30) = %.0f GB/s at 8 B per weight" % (us_a, n * 8 / us_a / 1e3))
    print("rsu_grad_accumulate add (gsum += g):    %.1f us (median of 30) = %.0f GB/s at 12 B per weight" % (us_s, n * 12 / us_s / 1e3))
    print("rsu_ema_step:                           %.1f us (median of 30) = %.0f GB/s at 12 B per weight" % (us_e, n * 12 / us_e / 1e3))
    print("a step of K micro-batches issues one assign and K - 1 adds: %.1f us at K = 2, %.1f us at K = 4, back to back and hot in the "
          "caches; inside a step the gradient has just been written by the backward pass" % (us_a + us_s, us_a + 3 * us_s))
