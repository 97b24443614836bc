#!/usr/bin/env python3
"""Developer tool (GPU box): what DevicePatchPool.load_batch costs in front of a training step, per loader.

  bench_loader.py [--images N] [--reps R]
      config 2's shapes (B = 4, S = 572, P = 388) over a pool of N mirror-extended 608-pixel images, twelve arms in one process:
        loop plain, loop D4                the per-sample torch copies (the default path, unchanged)
        one launch plain, one launch D4    --one_launch_loader: one rsu_affine_patches call per batch
        one launch rot 180 scale 0.8-1.25  --random_rotation=180 --random_scale=0.8,1.25 --d4_augmentation
        + elastic 10 px on 3 cells         the same with --elastic_deformation=10,3: one rsu_elastic_patches call per batch instead
        + jitter, no contrast              --color_jitter=0.2,0,0.2,10: one rsu_color_jitter call behind the loader, one launch (apply)
        + jitter                           --color_jitter=0.2,0.2,0.2,10: two launches (sums, apply)
        + jitter + noise                   the same with --random_noise=0.02
      the three jitter arms once behind "loop plain" (rotation off) and once behind the rotation arm (rotation on).
      Per arm: the median of R event-timed load_batch calls (us, device time between two events on the stream: host-bound issue gaps
      of the loop arms are part of it, as they are in front of a training step), the host's own time inside the call, and GB/s at 24 B
      per input pixel (12 read, 12 written) plus 9 B per label (1 read, 8 written), plus 24 B per input pixel for the jitter's apply pass
      and 12 B for its sums pass -- to be read against the copy rate of profiles/*/hbm_rates.txt. Every pool is built and warmed first;
      then the arms ALTERNATE: repetition i times one batch of every arm in turn, so that a drift of the box moves all arms alike. Every
      arm cuts the same sequence of patches.
      Then the kernels alone: 50 back-to-back rsu_affine_patches / rsu_elastic_patches / rsu_color_jitter calls on prebuilt records between
      two events, per kind of record (the Python of load_batch -- the draws, the records -- is outside; what is left per call is one
      ctypes call and the launches); the loader's kinds ALTERNATE over seven rounds and the median round is reported. One elastic and
      one jittered batch are compared with hostio.elastic_patches / hostio.color_jitter at this size.
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
from road_segmentation_unet_amd.pool import DevicePatchPool, affine_draw, elastic_draw, jitter_draw  # noqa: E402

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

ROT = dict(augment=True, rotation=180.0, scale=(0.8, 1.25))
JITTERS = [("jitter, no contrast", dict(jitter=(0.2, 0.0, 0.2, 10.0))), ("jitter", dict(jitter=(0.2, 0.2, 0.2, 10.0))),
           ("jitter + noise", dict(jitter=(0.2, 0.2, 0.2, 10.0), noise=0.02))]
ARMS = [("loop plain", dict()), ("loop D4", dict(augment=True)), ("one launch plain", dict(one_launch=True)),
        ("one launch D4", dict(one_launch=True, augment=True)), ("one launch rot 180 scale 0.8-1.25", ROT)]
ELASTIC = (10.0, 3)
ARMS += [("rot 180 + elastic 10 px on 3 cells", dict(ROT, elastic=ELASTIC))]
ARMS += [("loop plain + " + n, dict(kw)) for n, kw in JITTERS] + [("rot 180 + " + n, dict(ROT, **kw)) for n, kw in JITTERS]


def arm_bytes(kw):
    jit = kw.get("jitter", (0.0,) * 4)
    extra = (24 if any(jit) or kw.get("noise", 0.0) else 0) + (12 if jit[1] else 0)
    return B * (S * S * (24 + extra) + P * P * 9)


WARM = 5
pools = [(name, kw, DevicePatchPool(ext, lab, S, P, STRIDE, device=DEV, seed=1, **kw)) for name, kw in ARMS]
order = np.random.RandomState(2).randint(0, len(pools[0][2]), size=(WARM + a.reps, B))
dev, host = {name: [] for name, _ in ARMS}, {name: [] for name, _ in ARMS}
for i, idx in enumerate(order):
    idx = [int(k) for k in idx]
    for name, kw, pl in pools:
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        t0 = time.perf_counter()
        pl.load_batch(idx, x, y)
        t1 = time.perf_counter()
        e.record()
        e.synchronize()
        if i >= WARM:
            dev[name].append(s.elapsed_time(e) * 1e3)
            host[name].append((t1 - t0) * 1e6)
us = {}
for name, kw, pl in pools:
    d = dev[name]
    us[name] = sorted(d)[len(d) // 2]
    print("%-34s %8.1f us (median of %d; min %.1f, max %.1f) = %6.0f GB/s; host inside the call %.1f us (median)"
          % (name + ":", us[name], len(d), min(d), max(d), arm_bytes(kw) / us[name] / 1e3, sorted(host[name])[len(d) // 2]))
print("one launch / loop: plain %.2f x, D4 %.2f x the loop's time; rotation and scale cost %.2f x the one-launch D4 batch"
      % (us["one launch plain"] / us["loop plain"], us["one launch D4"] / us["loop D4"],
         us["one launch rot 180 scale 0.8-1.25"] / us["one launch D4"]))
print("elastic deformation on top of the rotation arm: %+.1f us per batch (%.2f x)"
      % (us["rot 180 + elastic 10 px on 3 cells"] - us["one launch rot 180 scale 0.8-1.25"],
         us["rot 180 + elastic 10 px on 3 cells"] / us["one launch rot 180 scale 0.8-1.25"]))
print("jitter on top of its loader (us): " + "; ".join(
    "%s %+.1f rotation off, %+.1f rotation on" % (n, us["loop plain + " + n] - us["loop plain"],
                                                   us["rot 180 + " + n] - us["one launch rot 180 scale 0.8-1.25"]) for n, _ in JITTERS))
del pools

pl = DevicePatchPool(ext, lab, S, P, STRIDE, device=DEV, seed=1, one_launch=True, elastic=(0.0, ELASTIC[1]))
idx = [int(k) for k in np.random.RandomState(2).randint(0, len(pl), size=B)]
st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
ROTKW = dict(d4=True, rotation=180.0, scale=(0.8, 1.25))
KINDS = []
for name, kw, alpha in (("plain", dict(), 0.0), ("D4", dict(d4=True), 0.0), ("rot 180 scale 0.8-1.25", ROTKW, 0.0),
                        ("rot 180 + elastic 10 px on 3 cells", ROTKW, ELASTIC[0])):
    M = affine_draw(np.random.RandomState(3), B, **kw)
    if alpha > 0.0:
        recs = pl.elastic_records(idx, M, elastic_draw(np.random.RandomState(5), B, *ELASTIC))
        recs["alpha"] = alpha
        KINDS.append((name, "rsu_elastic_patches", recs, recs.ctypes.data_as(ctypes.POINTER(_lib.RsuElastic))))
    else:
        recs = pl.affine_records(idx, M)
        KINDS.append((name, "rsu_affine_patches", recs, recs.ctypes.data_as(ctypes.POINTER(_lib.RsuAffine))))


def loader_launch(entry, rp):
    _lib.call(entry, pl.dev_images.data_ptr(), pl.dev_labels.data_ptr(), rp, B, a.images, HE, HL, S, P, x.data_ptr(), y.data_ptr(), st)


ROUNDS = 7
alone = {name: [] for name, _, _, _ in KINDS}
for rnd in range(ROUNDS + 1):   # (round 0 warms every kind up and is dropped)
    for name, entry, recs, rp in KINDS:
        torch.cuda.synchronize()
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(50):
            loader_launch(entry, rp)
        e.record()
        e.synchronize()
        if rnd:
            alone[name].append(s.elapsed_time(e) * 1e3 / 50)
for name, entry, recs, rp in KINDS:
    t = sorted(alone[name])[ROUNDS // 2]
    print("kernel alone, %-36s %6.1f us per call (median of %d alternated rounds of 50 calls back to back; min %.1f, max %.1f) = %6.0f GB/s"
          % (name + ":", t, ROUNDS, min(alone[name]), max(alone[name]), nbytes / t / 1e3))
name, entry, recs, rp = KINDS[-1]
loader_launch(entry, rp)
torch.cuda.synchronize()
hx, hy = hostio.elastic_patches(ext, lab, recs, S, P)
print("    one elastic batch equals hostio.elastic_patches at %d x %d^2: inputs %s, labels %s"
      % (B, S, np.array_equal(x.cpu().numpy().view(np.int32), hx.view(np.int32)), np.array_equal(y.cpu().numpy(), hy)))

# the jitter's kernels alone, on the batch the last loader call left in x (restored before every call would cost a copy: the values drift to
# the clamp over 55 calls, which changes no instruction count -- the kernels have no data-dependent branch)
ws = torch.empty(_lib.lib().rsu_color_jitter_ws_bytes(B, S) // 8, dtype=torch.int64, device=DEV)
for name, kw in JITTERS:
    recs = jitter_draw(np.random.RandomState(4), B, *kw["jitter"], noise=kw.get("noise", 0.0))
    rp = recs.ctypes.data_as(ctypes.POINTER(_lib.RsuJitter))
    nb = B * S * S * (24 + (12 if kw["jitter"][1] else 0))

    def launch():
        _lib.call("rsu_color_jitter", x.data_ptr(), rp, B, S, ws.data_ptr(), st)
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
    print("rsu_color_jitter alone, %-20s %6.1f us per call (50 calls back to back; %d launch%s per call) = %6.0f GB/s at %.1f MB"
          % (name + ":", t, 2 if kw["jitter"][1] else 1, "es" if kw["jitter"][1] else "", nb / t / 1e3, nb / 1e6))
    pl.load_batch(idx, x, y)
    torch.cuda.synchronize()
    before = x.cpu().numpy()
    launch()
    torch.cuda.synchronize()
    print("    one batch of this kind equals hostio.color_jitter at %d x %d^2: %s" % (B, S, np.array_equal(x.cpu().numpy(), hostio.color_jitter(before, recs))))
