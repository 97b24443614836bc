#!/usr/bin/env python3
"""Developer tool (GPU box): what --weight_decay costs.

  bench_decay.py pass
      the update pass alone at config 2's table, in one process, arms alternated: the plain entry (rsu_update_table_run /
      rsu_update_table_run_adam) against the decaying entry of include/rsu_optim.h in both modes, for both optimizers: us per call
      (median of 30 per arm, the arms taking turns call by call) and GB/s at 24 B (Momentum) / 32 B (Adam) per weight.
  bench_decay.py step [--tree PARENT] [--reps N]
      the config-2 training step, for both optimizers, under the arms off / decoupled / l2 (and, with --tree, the parent commit's
      built checkout PARENT with its own library as a fourth arm), alternating fresh processes on one box (the pattern of
      tools/bench_ema.py). Every process runs under its own time limit and the series stops at the first one that fails. Medians per
      arm; the spread of the parent arm's runs (without --tree: of the off arm's) is the noise the differences are read against.
  bench_decay.py arm [--tree DIR] [--decay LAMBDA] [--mode decoupled|l2] [--optimizer momentum|adam] [--steps N]
      one arm of the above in this process: L = 5, root 64, 388 px, 4 patches; forward + backward + update on a fixed batch, dropout
      off as in bench.py; ms per step over N steps between two events after 10 warm-up steps. --tree DIR imports the package from
      another checkout (it needs --decay 0: the keyword does not exist in the parent).
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
ap.add_argument("mode_", metavar="mode", choices=["pass", "step", "arm"])
ap.add_argument("--tree", default=None)
ap.add_argument("--decay", type=float, default=0.0)
ap.add_argument("--mode", default="decoupled")
ap.add_argument("--optimizer", default="momentum")
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--reps", type=int, default=3)
a = ap.parse_args()


def median(v):
    return sorted(v)[len(v) // 2]


if a.mode_ == "step":
    arms = ([("parent", ["--tree", a.tree, "--decay", "0"])] if a.tree else []) + \
        [("off", ["--decay", "0"]), ("decoupled", ["--decay", "1e-4", "--mode", "decoupled"]), ("l2", ["--decay", "1e-4", "--mode", "l2"])]
    for optimizer in ("momentum", "adam"):
        ms = {k: [] for k, _ in arms}
        for rep in range(a.reps):
            for name, extra in arms:
                cmd = ["timeout", "-k", "10", "150", sys.executable, os.path.abspath(__file__), "arm", "--optimizer", optimizer,
                       "--steps", str(a.steps)] + extra
                r = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True)
                sys.stdout.write(r.stdout)
                sys.stdout.flush()
                m = re.search(r": ([0-9.]+) ms/step", r.stdout)
                if r.returncode != 0 or not m:
                    sys.exit("arm %s failed (exit status %d): the series stops here" % (name, r.returncode))
                ms[name].append(float(m.group(1)))
        med = {k: median(v) for k, v in ms.items()}
        for k, _ in arms:
            print("%-9s %-9s ms/step: %s | median %.4f min %.4f max %.4f" % (optimizer, k, " ".join("%.4f" % v for v in ms[k]), med[k],
                                                                            min(ms[k]), max(ms[k])))
        base = "parent" if a.tree else "off"
        spread = max(ms[base]) - min(ms[base])
        print("%s: the %s arm's run-to-run spread (max - min): %.4f ms" % (optimizer, base, spread))
        if a.tree:
            d = med["off"] - med["parent"]
            print("%s: decay off - parent (medians): %+.4f ms (%+.2f %%): %s the parent's spread" % (optimizer, d, 100 * d / med["parent"],
                                                                                                    "inside" if abs(d) <= spread else "OUTSIDE"))
        for k in ("decoupled", "l2"):
            d = med[k] - med["off"]
            print("%s: %s - off (medians): %+.4f ms (%+.2f %%) per step" % (optimizer, k, d, 100 * d / med["off"]))
    sys.exit(0)

sys.path.insert(0, os.path.abspath(a.tree or HERE))

import numpy as np  # noqa: E402
import torch  # noqa: E402
from road_segmentation_unet_amd import _lib  # noqa: E402
from road_segmentation_unet_amd.unet import UNet, _ptr  # noqa: E402

L, ROOT_SIZE, DIL, B, P = 5, 64, False, 4, 388
sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]


def net(optimizer, **kw):
    m = UNet(L, ROOT_SIZE, DIL, B, P, training=True, optimizer=optimizer, **kw)
    gen = torch.Generator(device="cpu").manual_seed(0)
    m.x.copy_(torch.rand((B, m.S, m.S, 3), generator=gen))
    m.labels.copy_((torch.rand((B, P, P), generator=gen) < 0.2).to(torch.int64))
    return m


if a.mode_ == "arm":
    m = net(a.optimizer, **({"weight_decay": a.decay, "weight_decay_mode": a.mode} if a.decay > 0 else {}))
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
    print("step %s decay %g %s tree %s lib %s: %.4f ms/step = %.1f patches/s (%d steps)"
          % (a.optimizer, a.decay, a.mode if a.decay > 0 else "-", os.path.basename(os.path.abspath(a.tree or HERE)), sha, ms, B / ms * 1e3, a.steps))
else:
    print("lib %s, device %s" % (sha, torch.cuda.get_device_name(0)))
    st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
    for optimizer in ("momentum", "adam"):
        m = net(optimizer)
        m.flat_g.normal_(0, 1e-3)
        tab = m._update_table or m._build_update_table()
        t = (_ptr(tab[0]), tab[1], tab[2])
        decays, live = m.decaying_parameters()
        d = float(np.float32(1e-3) * np.float32(1e-4))
        if optimizer == "adam":
            rule = (1e-4, 0.9, 0.999, 1e-8, 1.0)
            arms = [("plain", lambda: _lib.call("rsu_update_table_run_adam", *t, *rule, st())),
                    ("decoupled", lambda: _lib.call("rsu_update_table_run_adam_decay", *t, *rule, d, _lib.DECAY_DECOUPLED, None, st())),
                    ("l2", lambda: _lib.call("rsu_update_table_run_adam_decay", *t, *rule, 1e-4, _lib.DECAY_L2, None, st()))]
        else:
            rule = (1e-3, 0.9, 1.0)
            arms = [("plain", lambda: _lib.call("rsu_update_table_run", *t, *rule, st())),
                    ("decoupled", lambda: _lib.call("rsu_update_table_run_decay", *t, *rule, d, _lib.DECAY_DECOUPLED, None, st())),
                    ("l2", lambda: _lib.call("rsu_update_table_run_decay", *t, *rule, 1e-4, _lib.DECAY_L2, None, st()))]
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
        bpw = 32 if optimizer == "adam" else 24
        print("%s: %d live weights, %d of them in packed kernels (they decay), %d workgroups" % (optimizer, live, decays, tab[2]))
        for name, _fn in arms:
            u = median(us[name])
            print("  %-9s %.1f us (median of 30, min %.1f max %.1f) = %.0f GB/s at %d B per weight; against plain %+.1f us (%+.2f %%)"
                  % (name, u, min(us[name]), max(us[name]), live * bpw / u / 1e3, bpw, u - median(us["plain"]),
                     100 * (u - median(us["plain"])) / median(us["plain"])))
