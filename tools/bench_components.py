#!/usr/bin/env python3
"""Developer tool (GPU box): what connected-component labelling on the device (include/rsu_components.h) costs, and what it saves.

  bench_components.py kernels
      rsu_components_label (with area and edge), rsu_components_filter (min_area 20, max_hole 20) and rsu_components_pair_count at
      2 x 608 x 608 and 2 x 388 x 388 against the route a user has without them, on the same device tensor: device-to-host copy,
      scipy.ndimage.label plus numpy.bincount per image, host-to-device copy of the areas. Inputs: a smooth road-like map (blurred
      noise through a sigmoid) and the test bank's rand0.55. One process, the arms alternated call by call; every call is timed on
      the host between two synchronisations (the scipy arm is host work): us per call, median of 20 rounds with min and max.
  bench_components.py step --lib PARENT_LIBRARY [--reps N] [--no-predict]
      the DEFAULT config-2 training step and the DEFAULT prediction of one 608 x 608 image (no flag of this change set) with this
      tree's library against the parent commit's library (built as `make -C road_segmentation_unet_amd/csrc VARIANT=parent` in a
      checkout of the parent, loaded through RSU_LIB_PATH), alternating fresh processes on one box; the order of the arms rotates from
      round to round. Every process runs under its own time limit and the series stops at the first one that fails. Medians per arm;
      the spread of the parent arm's runs is the noise the difference is read against.
  bench_components.py arm [--predict] [--steps N]
      one arm of the above in this process. --parent-lib: the library is the parent commit's, which has no entry of
      rsu_components.h -- the table is left unbound (the default step and prediction call none of them).
The record goes to standard output: keep it under profiles/rNN/.
"""
import argparse
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
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--predict", action="store_true")
ap.add_argument("--no-predict", action="store_true", help="step: leave the two prediction arms out")
ap.add_argument("--parent-lib", action="store_true")
a = ap.parse_args()


def median(v):
    return sorted(v)[len(v) // 2]


if a.mode_ == "step":
    if not a.lib or not os.path.exists(a.lib):
        sys.exit("step needs --lib: the parent commit's library")
    parent = {"RSU_LIB_PATH": os.path.abspath(a.lib)}
    arms = [("parent step", parent, ["--parent-lib"]), ("this step", {}, []), ("parent predict", parent, ["--parent-lib", "--predict"]),
            ("this predict", {}, ["--predict"])]
    if a.no_predict:
        arms = arms[:2]
    ms = {k: [] for k, _, _ in arms}
    for rep in range(a.reps):
        for name, env, extra in arms[rep % len(arms):] + arms[:rep % len(arms)]:   # (no arm is always the first of its round)
            cmd = ["timeout", "-k", "10", "200", sys.executable, os.path.abspath(__file__), "arm", "--steps", str(a.steps)] + extra
            e = {k: v for k, v in os.environ.items() if k != "RSU_LIB_PATH"}
            e.update(env)
            r = subprocess.run(cmd, stdout=subprocess.PIPE, universal_newlines=True, env=e)
            sys.stdout.write(r.stdout)
            sys.stdout.flush()
            m = re.search(r": ([0-9.]+) ms/(step|image)", r.stdout)
            if r.returncode != 0 or not m:
                sys.exit("arm %s failed (exit status %d): the series stops here" % (name, r.returncode))
            ms[name].append(float(m.group(1)))
    med = {k: median(v) for k, v in ms.items()}
    for k, _, _ in arms:
        print("%-14s ms: %s | median %.4f min %.4f max %.4f" % (k, " ".join("%.4f" % v for v in ms[k]), med[k], min(ms[k]), max(ms[k])))
    for what in ("step",) if a.no_predict else ("step", "predict"):
        spread = max(ms["parent " + what]) - min(ms["parent " + what])
        d = med["this " + what] - med["parent " + what]
        print("default %s, this library - parent's (medians): %+.4f ms (%+.2f %%); the parent arm's run-to-run spread (max - min) %.4f ms: %s it"
              % (what, d, 100 * d / med["parent " + what], spread, "inside" if abs(d) <= spread else "OUTSIDE"))
    sys.exit(0)

sys.path.insert(0, HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as Fn  # noqa: E402
from road_segmentation_unet_amd import _lib  # noqa: E402
from road_segmentation_unet_amd.unet import UNet, _ptr  # noqa: E402

if a.parent_lib:
    _lib.SIGNATURES_COMPONENTS.clear()
sha = hashlib.sha256(open(_lib.LIB_PATH, "rb").read()).hexdigest()[:16]

if a.mode_ == "arm" and not a.predict:
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
    opts = Options(num_layers=5, root_size=64, patch_size=388, stride=44, batch_size=8, dropout=1.0, logdir=None)
    model = ConvolutionalModel(opts)
    imgs = np.random.RandomState(0).rand(1, 608, 608, 3).astype(np.float32)
    model.predict(imgs)
    model.predict(imgs)
    t = []
    for _ in range(5):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        masks = model.predict(imgs)
        torch.cuda.synchronize(); t.append((time.perf_counter() - t0) * 1e3)
    print("default predict lib %s, 608 x 608, stride 44, 6-way ensemble, 5 calls %s: %.4f ms/image (median)"
          % (sha, " ".join("%.1f" % v for v in t), median(t)))
    sys.exit(0)

# ---- kernels
print("lib %s, device %s" % (sha, torch.cuda.get_device_name(0)))
dev = "cuda:0"
lib = _lib.lib()
st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
THR, CONN, MIN_AREA, MAX_HOLE = 0.5, 8, 20, 20


def inputs(N, S):
    gen = torch.Generator(device="cpu").manual_seed(1)
    noise = torch.randn((N, 1, S, S), generator=gen)
    for _ in range(6):
        noise = Fn.avg_pool2d(noise, 5, 1, 2)
    smooth = torch.sigmoid(noise[:, 0] / noise.std() * 3.0 - 1.0).contiguous()
    rnd = torch.from_numpy(np.where(np.random.RandomState(7).random_sample((N, S, S)) < 0.55, 0.75, 0.25).astype(np.float32))
    return [("smooth road-like map", smooth), ("rand0.55", rnd)]


class Case:
    def __init__(self, prob):
        self.N, self.H, self.W = (int(v) for v in prob.shape)
        self.prob = prob.to(dev)
        self.labels = torch.zeros(prob.shape, dtype=torch.int32, device=dev)
        self.area = torch.zeros(prob.shape, dtype=torch.int32, device=dev)
        self.edge = torch.zeros(prob.shape, dtype=torch.uint8, device=dev)
        self.out = torch.zeros(prob.shape, dtype=torch.float32, device=dev)
        self.stats = torch.zeros((self.N, 6), dtype=torch.int64, device=dev)
        self.acc = torch.zeros(4, dtype=torch.int64, device=dev)
        self.lab64 = (self.prob >= 0.6).to(torch.int64)
        self.ws = torch.zeros(lib.rsu_components_ws_bytes(self.N, self.H, self.W) // 4, dtype=torch.int32, device=dev)
        self.scipy_area = None

    def label(self):
        _lib.call("rsu_components_label", _ptr(self.prob), THR, CONN, 0, _ptr(self.labels), _ptr(self.area), _ptr(self.edge), _ptr(self.ws),
                  self.N, self.H, self.W, st())

    def filter(self):
        _lib.call("rsu_components_filter", _ptr(self.prob), THR, CONN, MIN_AREA, MAX_HOLE, _ptr(self.out), _ptr(self.stats), _ptr(self.ws),
                  self.N, self.H, self.W, st())

    def pair(self):
        _lib.call("rsu_components_pair_count", _ptr(self.prob), THR, _ptr(self.lab64), CONN, _ptr(self.acc), _ptr(self.ws), self.N, self.H,
                  self.W, st())

    def scipy_route(self):
        """what a user does today: copy to the host, label and count every image, copy the per-pixel areas back"""
        from scipy import ndimage
        p = self.prob.cpu().numpy()
        areas = np.empty(p.shape, np.int32)
        for n in range(self.N):
            lab, _k = ndimage.label(p[n] >= THR, structure=np.ones((3, 3), int))
            areas[n] = np.bincount(lab.reshape(-1))[lab] * (lab > 0)
        self.scipy_area = torch.from_numpy(areas).to(dev)


def timed(arms, rounds=20):
    for _ in range(3):
        for _n, fn in arms:
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k, _ in arms}
    for _ in range(rounds):
        for name, fn in arms:
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(); us[name].append((time.perf_counter() - t0) * 1e6)
    return us


for S in (608, 388):
    for name, prob in inputs(2, S):
        c = Case(prob)
        print("N x H x W = 2 x %d x %d, %s, connectivity %d; us per call between two synchronisations, median of 20 (min .. max)" % (S, S, name, CONN))
        us = timed([("rsu_components_label", c.label), ("rsu_components_filter", c.filter), ("rsu_components_pair_count", c.pair),
                    ("copy + scipy + copy", c.scipy_route)])
        for arm, u in us.items():
            print("  %-26s %9.1f us (%.1f .. %.1f)" % (arm, median(u), min(u), max(u)))
        same = bool(torch.equal(c.area, c.scipy_area))
        lm, sm = median(us["rsu_components_label"]), median(us["copy + scipy + copy"])
        print("  components %d; areas equal scipy's: %s; label %.1f us against %.1f us: x %.1f" % (int((c.labels == torch.arange(
            1, S * S + 1, device=dev, dtype=torch.int32).reshape(1, S, S)).sum()), same, lm, sm, sm / lm))
        print("  filter stats (summed): %s" % c.stats.sum(0).tolist())
