#!/usr/bin/env python3
"""Developer tool (GPU box): what --clip_grad_norm costs. One process times one arm; an A/B alternates processes (tools/clip_ab.sh).

  bench_clip.py step [--tree DIR] [--clip C] [--optimizer momentum|adam] [--steps N]
      the config-2 training step (L = 5, root 64, 388 px, 4 patches; forward + backward + update on a fixed batch, dropout off as in
      bench.py), ms per step over N steps between two events after 10 warm-up steps. --tree DIR imports the package from another
      checkout (the parent commit's, with its own library: the A side of the A/B; it needs --clip 0, the keyword does not exist there).
      --clip 0: a net built without clip_grad_norm.
  bench_clip.py norm
      rsu_grad_norm alone on the config-2 gradient: us per call (median of 30) and GB/s at 4 B per live weight -- to be read against
      the read-only rate of profiles/r06/hbm_rates.txt -- and the clipping update pass next to the plain one.
"""
import argparse
import hashlib
import os
import sys

ap = argparse.ArgumentParser()
ap.add_argument("mode", choices=["step", "norm"])
ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--clip", type=float, default=0.0)
ap.add_argument("--optimizer", default="momentum")
ap.add_argument("--steps", type=int, default=60)
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.tree))

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


def net(clip, optimizer):
    kw = {"clip_grad_norm": clip} if clip > 0 else {}
    m = UNet(L, ROOT_SIZE, DIL, B, P, training=True, optimizer=optimizer, **kw)
    gen = torch.Generator(device="cpu").manual_seed(0)
    m.x.copy_(torch.rand((B, m.S, m.S, 3), generator=gen))
    m.labels.copy_((torch.rand((B, P, P), generator=gen) < 0.2).to(torch.int64))
    return m


if a.mode == "step":
    m = net(a.clip, a.optimizer)
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
    extra = ""
    if a.clip > 0:
        st = m.clip_stats()
        extra = " | clip steps %d clipped %d skipped %d last norm %.4g" % (st["steps"], st["clipped"], st["skipped"], st["norm"])
    print("step %s clip %g tree %s lib %s: %.4f ms/step = %.1f patches/s (%d steps)%s"
          % (a.optimizer, a.clip, os.path.basename(os.path.abspath(a.tree)), sha, ms, B / ms * 1e3, a.steps, extra))
else:
    m = net(1e30, a.optimizer)
    m.flat_g.normal_(0, 1e-3)
    plain = net(0.0, a.optimizer)
    plain.flat_g.copy_(m.flat_g)
    us = median_us(m._grad_norm)
    print("lib %s, %d live weights (%.1f MB of gradient)" % (sha, m.n_live, m.n_live * 4 / 1e6))
    print("rsu_grad_norm (both launches): %.1f us (median of 30) = %.0f GB/s at 4 B per weight" % (us, m.n_live * 4 / us / 1e3))
    up = (lambda n: n.apply_adam(0.0)) if a.optimizer == "adam" else (lambda n: n.apply_momentum(0.0, 0.9))
    u_clip, u_plain = median_us(lambda: up(m)), median_us(lambda: up(plain))
    print("%s update: plain pass %.1f us, norm + clipping pass %.1f us (+%.1f us)" % (a.optimizer, u_plain, u_clip, u_clip - u_plain))
