#!/usr/bin/env python3
"""Developer tool (GPU box): what DevicePatchPool.load_batch costs in front of a training step, per loader.

  bench_loader.py [--images N] [--reps R]
      config 2's shapes (B = 4, S = 572, P = 388) over a pool of N mirror-extended 608-pixel images, five arms in one process:
        loop plain, loop D4                the per-sample torch copies (the default path, unchanged)
        one launch plain, one launch D4    --one_launch_loader: one rsu_affine_patches call per batch
        one launch rot 180 scale 0.8-1.25  --random_rotation=180 --random_scale=0.8,1.25 --d4_augmentation
      Per arm: the median of R event-timed load_batch calls after warm-up (us, device time between two events on the stream: host-bound
      issue gaps of the loop arms are part of it, as they are in front of a training step), the host's own time inside the call, and
      GB/s at 24 B per input pixel (12 read, 12 written) plus 9 B per label (1 read, 8 written) -- to be read against the copy rate of
      profiles/*/hbm_rates.txt. Every arm cuts the same sequence of patches.
      Then the kernel alone: 50 back-to-back rsu_affine_patches calls on prebuilt records between two events, per kind of record (the
      Python of load_batch -- the draws, the records -- is outside; what is left per call is one ctypes call and the launch).
The record goes to standard output: keep it under profiles/rNN/.
"""
import argparse
import ctypes
import hashlib
import os
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
ap = argparse.ArgumentParser()
ap.add_argument("--images", type=int, default=6)
ap.add_argument("--reps", type=int, default=30)
a = ap.parse_args()

import numpy as np  # noqa: E402
import torch  # noqa: E402
from road_segmentation_unet_amd import _lib, hostio  # noqa: E402
from road_segmentation_unet_amd.pool import DevicePatchPool, affine_draw  # noqa: E402

B, S, P, HE, STRIDE = 4, 572, 388, 608, 12
OFFSET = (S - P) // 2
HL = HE - 2 * OFFSET
DEV = "cuda:0"
sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]
rng = np.random.RandomState(0)
ext = hostio.mirror_border(rng.rand(a.images, HL, HL, 3).astype(np.float32), OFFSET)
lab = (rng.rand(a.images, HL, HL) < 0.2).astype(np.uint8)
x = torch.empty((B, S, S, 3), dtype=torch.float32, device=DEV)
y = torch.empty((B, P, P), dtype=torch.int64, device=DEV)
nbytes = B * (S * S * 24 + P * P * 9)
print("lib %s, device %s; B %d, S %d, P %d, %d images of %d px (labels %d px), %.1f MB moved per batch"
      % (sha, torch.cuda.get_device_name(0), B, S, P, a.images, HE, HL, nbytes / 1e6))

ARMS = [("loop plain", dict()), ("loop D4", dict(augment=True)), ("one launch plain", dict(one_launch=True)),
        ("one launch D4", dict(one_launch=True, augment=True)),
        ("one launch rot 180 scale 0.8-1.25", dict(augment=True, rotation=180.0, scale=(0.8, 1.25)))]
WARM = 5
us = {}
for name, kw in ARMS:
    pl = DevicePatchPool(ext, lab, S, P, STRIDE, device=DEV, seed=1, **kw)
    order = np.random.RandomState(2).randint(0, len(pl), size=(WARM + a.reps, B))
    dev, host = [], []
    for i, idx in enumerate(order):
        idx = [int(k) for k in idx]
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        t0 = time.perf_counter()
        pl.load_batch(idx, x, y)
        t1 = time.perf_counter()
        e.record()
        e.synchronize()
        if i >= WARM:
            dev.append(s.elapsed_time(e) * 1e3)
            host.append((t1 - t0) * 1e6)
    us[name] = sorted(dev)[len(dev) // 2]
    print("%-34s %8.1f us (median of %d; min %.1f, max %.1f) = %6.0f GB/s; host inside the call %.1f us (median)"
          % (name + ":", us[name], len(dev), min(dev), max(dev), nbytes / us[name] / 1e3, sorted(host)[len(host) // 2]))
print("one launch / loop: plain %.2f x, D4 %.2f x the loop's time; rotation and scale cost %.2f x the one-launch D4 batch"
      % (us["one launch plain"] / us["loop plain"], us["one launch D4"] / us["loop D4"],
         us["one launch rot 180 scale 0.8-1.25"] / us["one launch D4"]))

pl = DevicePatchPool(ext, lab, S, P, STRIDE, device=DEV, seed=1, one_launch=True)
idx = [int(k) for k in np.random.RandomState(2).randint(0, len(pl), size=B)]
st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
for name, kw in (("plain", dict()), ("D4", dict(d4=True)), ("rot 180 scale 0.8-1.25", dict(d4=True, rotation=180.0, scale=(0.8, 1.25)))):
    recs = pl.affine_records(idx, affine_draw(np.random.RandomState(3), B, **kw))
    rp = recs.ctypes.data_as(ctypes.POINTER(_lib.RsuAffine))

    def launch():
        _lib.call("rsu_affine_patches", pl.dev_images.data_ptr(), pl.dev_labels.data_ptr(), rp, B, a.images, HE, HL, S, P, x.data_ptr(),
                  y.data_ptr(), st)
    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(50):
        launch()
    e.record()
    e.synchronize()
    t = s.elapsed_time(e) * 1e3 / 50
    print("kernel alone, %-24s %6.1f us per call (50 calls back to back) = %6.0f GB/s" % (name + ":", t, nbytes / t / 1e3))
