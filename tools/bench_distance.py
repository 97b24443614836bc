#!/usr/bin/env python3
"""Developer tool (GPU box): what the mask distances on the device (include/rsu_distance.h) cost, and what they save.

  bench_distance.py kernels [--row-libs ROWS=LIBRARY,ROWS=LIBRARY,...]
      rsu_distance_hist and rsu_mask_distance (both outputs) at 2 x 388 x 388 and 2 x 608 x 608 against the route a user has without
      them, on the same device tensors: device-to-host copy of the probabilities and the labels, two
      scipy.ndimage.distance_transform_edt per image, numpy.bincount of the rounded-up distances. Inputs: a smooth road-like map
      (blurred noise through a sigmoid; the truth is the same map at a higher level, so the prediction is the truth grown by a few
      pixels) and the test bank's random pair (rand0.55 against rand0.41: every distance is 0, 1 or 2 pixels). One process, the arms
      alternated call by call; every call is timed on the host between two synchronisations (the scipy arm is host work): us per call,
      median of 20 rounds with min and max (the scipy arm: 3 rounds). --row-libs: A/B builds of the library that differ in the rows a workgroup of the histogram's
      row launch takes (make -C road_segmentation_unet_amd/csrc VARIANT=rowsK EXTRA=-DDT_HIST_ROWS=K); rsu_distance_hist and
      rsu_mask_distance of each are timed in the same alternation, and every arm's outputs must equal the first's.
  bench_distance.py step --lib PARENT_LIBRARY [--reps N]
      the DEFAULT config-2 training step and a DEFAULT validation pass (evaluate() over 8 patches of 388 x 388, no flag of this change
      set) with this tree's library against the parent commit's library (built as `make -C road_segmentation_unet_amd/csrc
      VARIANT=parent` in a checkout of the parent, loaded through RSU_LIB_PATH), alternating fresh processes on one box; the order of the
      arms rotates from round to round. Every process runs under its own time limit and the series stops at the first one that fails.
      Medians per arm; the spread of the parent arm's runs is the noise the difference is read against.
  bench_distance.py arm [--validate] [--steps N]
      one arm of the above in this process. --parent-lib: the library is the parent commit's, which has no entry of rsu_distance.h --
      the table is left unbound (the default step and validation call none of them).
The record goes to standard output: keep it under profiles/rNN/.
"""
import argparse
import ctypes
import hashlib
import os
import re
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ap = argparse.ArgumentParser()
ap.add_argument("mode_", metavar="mode", choices=["kernels", "step", "arm"])
ap.add_argument("--lib", default=None)
ap.add_argument("--row-libs", default="")
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--validate", action="store_true")
ap.add_argument("--parent-lib", action="store_true")
a = ap.parse_args()


def median(v):
    return sorted(v)[len(v) // 2]


if a.mode_ == "step":
    if not a.lib or not os.path.exists(a.lib):
        sys.exit("step needs --lib: the parent commit's library")
    parent = {"RSU_LIB_PATH": os.path.abspath(a.lib)}
    arms = [("parent step", parent, ["--parent-lib"]), ("this step", {}, []), ("parent validate", parent, ["--parent-lib", "--validate"]),
            ("this validate", {}, ["--validate"])]
    ms = {k: [] for k, _, _ in arms}
    for rep in range(a.reps):
        for name, env, extra in arms[rep % len(arms):] + arms[:rep % len(arms)]:   # (no arm is always the first of its round)
            cmd = ["timeout", "-k", "10", "200", sys.executable, os.path.abspath(__file__), "arm", "--steps", str(a.steps)] + extra
            e = {k: v for k, v in os.environ.items() if k != "RSU_LIB_PATH"}
            e.update(env)
            r = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True, env=e)
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            m = re.search(r": ([0-9.]+) ms/(step|pass)", r.stdout)
            if r.returncode != 0 or not m:
                sys.exit("arm %s failed (exit status %d): the series stops here" % (name, r.returncode))
            ms[name].append(float(m.group(1)))
    med = {k: median(v) for k, v in ms.items()}
    for k, _, _ in arms:
        print("%-15s ms: %s | median %.4f min %.4f max %.4f" % (k, " ".join("%.4f" % v for v in ms[k]), med[k], min(ms[k]), max(ms[k])))
    for what in ("step", "validate"):
        spread, own = max(ms["parent " + what]) - min(ms["parent " + what]), max(ms["this " + what]) - min(ms["this " + what])
        d = med["this " + what] - med["parent " + what]
        print("default %s, this library - parent's (medians): %+.4f ms (%+.2f %%); run-to-run spread (max - min) of the parent arm %.4f ms, of "
              "this arm %.4f ms: %s the parent's" % (what, d, 100 * d / med["parent " + what], spread, own,
                                                     "inside" if abs(d) <= spread else "OUTSIDE"))
    sys.exit(0)

sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as Fn  # noqa: E402
from road_segmentation_unet_amd import _lib  # noqa: E402
from road_segmentation_unet_amd.unet import UNet, _ptr  # noqa: E402

if a.parent_lib:
    _lib.SIGNATURES_DISTANCE.clear()
sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]

if a.mode_ == "arm" and not a.validate:
    L, ROOT_SIZE, DIL, B, P = 5, 64, False, 4, 388
    m = UNet(L, ROOT_SIZE, DIL, B, P, training=True)
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
    print("default step lib %s: %.4f ms/step = %.1f patches/s (%d steps)" % (sha, ms, B / ms * 1e3, a.steps))
    sys.exit(0)

if a.mode_ == "arm":
    from road_segmentation_unet_amd.model import ConvolutionalModel, Options
    from road_segmentation_unet_amd.unet import input_size_needed
    opts = Options(num_layers=5, root_size=64, patch_size=388, batch_size=4, dropout=1.0, logdir=None)
    model = ConvolutionalModel(opts)
    rng = np.random.RandomState(0)
    S = input_size_needed(388, 5)
    X, y = rng.rand(8, S, S, 3).astype(np.float32), (rng.rand(8, 388, 388) < 0.2).astype(np.int64)
    model.evaluate(X, y)
    model.evaluate(X, y)
    t = []
    for _ in range(7):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        v = model.evaluate(X, y)
        torch.cuda.synchronize(); t.append((time.perf_counter() - t0) * 1e3)
    assert "dist_hist" not in v
    print("default validate lib %s, 8 patches of 388 x 388 in chunks of 4, 7 calls %s: %.4f ms/pass (median)"
          % (sha, " ".join("%.1f" % x for x in t), median(t)))
    sys.exit(0)

# ---- kernels
print("lib %s, device %s" % (sha, torch.cuda.get_device_name(0)))
dev = "cuda:0"
lib = _lib.lib()
st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
THR, BINS = 0.5, _lib.DIST_BINS
row_libs = []
for item in [s for s in a.row_libs.split(",") if s]:
    rows, path = item.split("=", 1)
    L = ctypes.CDLL(os.path.abspath(path))
    for entry in ("rsu_distance_hist", "rsu_mask_distance"):
        getattr(L, entry).restype, getattr(L, entry).argtypes = _lib.SIGNATURES_DISTANCE[entry]
    row_libs.append((int(rows), L, hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]))
for rows, _L, h in row_libs:
    print("row-block variant: %d row(s) per workgroup, lib %s" % (rows, h))


def inputs(N, S):
    gen = torch.Generator(device="cpu").manual_seed(1)
    noise = torch.randn((N, 1, S, S), generator=gen)
    for _ in range(6):
        noise = Fn.avg_pool2d(noise, 5, 1, 2)
    smooth = torch.sigmoid(noise[:, 0] / noise.std() * 3.0 - 1.0).contiguous()
    rs = np.random.RandomState(7)
    rnd = torch.from_numpy(np.where(rs.random_sample((N, S, S)) < 0.55, 0.75, 0.25).astype(np.float32))
    rnd_true = torch.from_numpy((np.random.RandomState(7).random_sample((N, S, S)) < 0.41).astype(np.int64))
    return [("smooth road-like map (truth: the map >= 0.6)", smooth, (smooth >= 0.6).to(torch.int64)),
            ("the test bank's random pair (rand0.55 against rand0.41)", rnd, rnd_true)]


class Case:
    def __init__(self, prob, lab64):
        self.N, self.H, self.W = (int(v) for v in prob.shape)
        self.prob, self.lab64 = prob.to(dev), lab64.to(dev)
        self.d2p = torch.zeros(prob.shape, dtype=torch.int32, device=dev)
        self.d2t = torch.zeros(prob.shape, dtype=torch.int32, device=dev)
        self.acc = torch.zeros((2, BINS), dtype=torch.int64, device=dev)
        self.row_acc = {rows: torch.zeros((2, BINS), dtype=torch.int64, device=dev) for rows, _L, _h in row_libs}
        self.row_d2 = {rows: torch.zeros((2,) + tuple(prob.shape), dtype=torch.int32, device=dev) for rows, _L, _h in row_libs}
        self.ws = torch.zeros(lib.rsu_distance_ws_bytes(self.N, self.H, self.W) // 4, dtype=torch.int32, device=dev)
        self.scipy_hist = self.scipy_d2 = None

    def hist(self):
        self.acc.zero_()
        _lib.call("rsu_distance_hist", _ptr(self.prob), THR, _ptr(self.lab64), _ptr(self.acc), _ptr(self.ws), self.N, self.H, self.W, st())

    def hist_of(self, rows, L):
        def run():
            self.row_acc[rows].zero_()
            rc = L.rsu_distance_hist(_ptr(self.prob), THR, _ptr(self.lab64), _ptr(self.row_acc[rows]), _ptr(self.ws), self.N, self.H, self.W, st())
            assert rc == 0, rc
        return run

    def distance_of(self, rows, L):
        def run():
            d2 = self.row_d2[rows]
            rc = L.rsu_mask_distance(_ptr(self.prob), THR, _ptr(self.lab64), _ptr(d2[0]), _ptr(d2[1]), _ptr(self.ws), self.N, self.H, self.W, st())
            assert rc == 0, rc
        return run

    def distance(self):
        _lib.call("rsu_mask_distance", _ptr(self.prob), THR, _ptr(self.lab64), _ptr(self.d2p), _ptr(self.d2t), _ptr(self.ws), self.N, self.H,
                  self.W, st())

    def scipy_route(self):
        """what a user does today: copy to the host, two distance transforms per image, the histogram of the rounded-up distances"""
        from scipy import ndimage
        p, y = self.prob.cpu().numpy(), self.lab64.cpu().numpy()
        hist = np.zeros((2, BINS), np.int64)
        d2 = np.empty((2,) + p.shape, np.int64)
        for n in range(self.N):
            pred, true = p[n] >= THR, y[n] == 1
            dt = ndimage.distance_transform_edt(~true) if true.any() else np.full(true.shape, 1e9)
            dp = ndimage.distance_transform_edt(~pred) if pred.any() else np.full(pred.shape, 1e9)
            d2[0, n], d2[1, n] = np.rint(dp * dp), np.rint(dt * dt)
            hist[0] += np.bincount(np.minimum(np.ceil(dt[pred] - 1e-9), BINS - 1).astype(np.int64), minlength=BINS)
            hist[1] += np.bincount(np.minimum(np.ceil(dp[true] - 1e-9), BINS - 1).astype(np.int64), minlength=BINS)
        self.scipy_hist, self.scipy_d2 = hist, d2


def timed(arms, rounds=20, slow="copy + 2 scipy edt + bincount", slow_rounds=3):
    """the host route is timed in the first rounds only: the arm behind it starts on a device that has idled for tens of milliseconds"""
    for _ in range(3):
        for _n, fn in arms:
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k, _ in arms}
    for r in range(rounds):
        for name, fn in arms:
            if name == slow and r >= slow_rounds:
                continue
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(); us[name].append((time.perf_counter() - t0) * 1e6)
    return us


for S in (388, 608):
    for name, prob, lab64 in inputs(2, S):
        c = Case(prob, lab64)
        print("N x H x W = 2 x %d x %d, %s; us per call between two synchronisations, median of 20 (min .. max)" % (S, S, name))
        arms = [("rsu_distance_hist", c.hist), ("rsu_mask_distance", c.distance), ("copy + 2 scipy edt + bincount", c.scipy_route)]
        arms += [("rsu_distance_hist, %d row(s)/workgroup" % rows, c.hist_of(rows, L)) for rows, L, _h in row_libs]
        arms += [("rsu_mask_distance, the %d-row library" % rows, c.distance_of(rows, L)) for rows, L, _h in row_libs]
        us = timed(arms)
        for arm, u in us.items():
            print("  %-38s %9.1f us (%.1f .. %.1f)" % (arm, median(u), min(u), max(u)))
        acc = c.acc.cpu().numpy()
        same_h = bool(np.array_equal(acc, c.scipy_hist))
        same_d = bool(np.array_equal(c.d2p.cpu().numpy(), c.scipy_d2[0]) and np.array_equal(c.d2t.cpu().numpy(), c.scipy_d2[1]))
        same_r = all(bool(np.array_equal(t.cpu().numpy(), acc)) for t in c.row_acc.values()) and \
            all(bool(torch.equal(t[0], c.d2p) and torch.equal(t[1], c.d2t)) for t in c.row_d2.values())
        hm, sm = median(us["rsu_distance_hist"]), median(us["copy + 2 scipy edt + bincount"])
        print("  histogram equals scipy's: %s; distances equal scipy's: %s; row-block variants agree: %s; hist %.1f us against %.1f us: x %.1f"
              % (same_h, same_d, same_r, hm, sm, sm / hm))
        print("  predicted pixels %d, true pixels %d; bins 0..7 of acc[0]: %s, last bin %d; of acc[1]: %s, last bin %d"
              % (acc[0].sum(), acc[1].sum(), acc[0, :8].tolist(), acc[0, -1], acc[1, :8].tolist(), acc[1, -1]))
