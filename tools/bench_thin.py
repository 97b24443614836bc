#!/usr/bin/env python3
"""Developer tool (GPU box): what the centre-line extraction on the device (include/rsu_thin.h) costs, and what it saves.

  bench_thin.py kernels [--k-libs K=LIBRARY,K=LIBRARY,...] [--iters N]
      rsu_mask_thin (both outputs, acc and info; --iters iterations at most, default 64) at 2 x 388 x 388 and 2 x 608 x 608 against the
      only route a user has without it, on the same device tensors: device-to-host copy of the probabilities and the labels,
      hostio.thin_mask of both masks -- a NUMPY RESTATEMENT of the same rule, not a library: no library thinning is installed -- and the
      copy of both skeletons back. Inputs: a smooth road-like map (blurred noise through a sigmoid; the truth is the same map at a
      higher level) and the test bank's random masks (rand0.55 against rand0.45). One process, the arms alternated call by call; every
      call is timed on the host between two synchronisations: us per call, median of 20 rounds with min and max (the numpy arm: 3
      rounds). --k-libs: A/B builds of the library that differ in the iterations a step launch carries
      (make -C road_segmentation_unet_amd/csrc VARIANT=thinK EXTRA=-DTH_K=K); each is timed in the same alternation with a workspace of
      its own size, and every arm's outputs must equal the first's. For every K the share of step launches that return early is
      derived from the iteration at which each image side stops changing (counted on the host): a side whose last deleting iteration
      is D works in 1 + ceil(D / K) of the ceil(iters / K) step launches.
  bench_thin.py step --lib PARENT_LIBRARY [--reps N]
      the DEFAULT config-2 training step and a DEFAULT validation pass (evaluate() over 8 patches of 388 x 388, no flag of this change
      set) with this tree's library against the parent commit's library (built as `make -C road_segmentation_unet_amd/csrc
      VARIANT=parent` in a checkout of the parent, loaded through RSU_LIB_PATH), alternating fresh processes on one box; the order of the
      arms rotates from round to round. Every process runs under its own time limit and the series stops at the first one that fails.
      Medians per arm; the spread of the parent arm's runs is the noise the difference is read against.
  bench_thin.py arm [--validate] [--steps N]
      one arm of the above in this process. --parent-lib: the library is the parent commit's, which has no entry of rsu_thin.h -- the
      table is left unbound (the default step and validation call none of them).
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
ap.add_argument("--k-libs", default="")
ap.add_argument("--iters", type=int, default=64)
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--reps", type=int, default=6)
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
from road_segmentation_unet_amd import _lib, hostio  # noqa: E402
from road_segmentation_unet_amd.unet import UNet, _ptr  # noqa: E402

if a.parent_lib:
    _lib.SIGNATURES_THIN.clear()
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
    assert "cl_hist" not in v
    print("default validate lib %s, 8 patches of 388 x 388 in chunks of 4, 7 calls %s: %.4f ms/pass (median)"
          % (sha, " ".join("%.1f" % x for x in t), median(t)))
    sys.exit(0)

# ---- kernels
print("lib %s, device %s, at most %d iterations" % (sha, torch.cuda.get_device_name(0), a.iters))
dev = "cuda:0"
lib = _lib.lib()
st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
THR = 0.5
src = open(os.path.join(HERE, "road_segmentation_unet_amd", "csrc", "thin.h")).read()
OWN_K = int(re.search(r"^#define TH_K (\d+)$", src, flags=re.M).group(1))
k_libs = []
for item in [s for s in a.k_libs.split(",") if s]:
    k, path = item.split("=", 1)
    L = ctypes.CDLL(os.path.abspath(path))
    for name in _lib.SIGNATURES_THIN:
        getattr(L, name).restype, getattr(L, name).argtypes = _lib.SIGNATURES_THIN[name]
    k_libs.append((int(k), L, hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]))
for k, _L, h in k_libs:
    print("variant: %d iteration(s) per step launch, lib %s" % (k, h))


def inputs(N, S):
    gen = torch.Generator(device="cpu").manual_seed(1)
    noise = torch.randn((N, 1, S, S), generator=gen)
    for _ in range(6):
        noise = Fn.avg_pool2d(noise, 5, 1, 2)
    smooth = torch.sigmoid(noise[:, 0] / noise.std() * 3.0 - 1.0).contiguous()
    rs = np.random.RandomState(7)
    rnd = torch.from_numpy(np.where(rs.random_sample((N, S, S)) < 0.55, 0.75, 0.25).astype(np.float32))
    rnd_true = torch.from_numpy((rs.random_sample((N, S, S)) < 0.45).astype(np.int64))
    return [("smooth road-like map (truth: the map >= 0.6)", smooth, (smooth >= 0.6).to(torch.int64)),
            ("the test bank's random masks (rand0.55 against rand0.45)", rnd, rnd_true)]


def last_deleting_iteration(mask):
    """per image: the last iteration of the rule that deletes a pixel (0: the mask is its own skeleton)"""
    m = mask.copy()
    last = np.zeros(m.shape[0], np.int64)
    for it in range(1, hostio.THIN_MAX_ITERS + 1):
        n = np.zeros(m.shape[0], np.int64)
        for sub in (0, 1):
            d = hostio._thin_deleted(m, sub)
            n += d.reshape(d.shape[0], -1).sum(axis=1)
            m &= ~d
        if not n.any():
            break
        last[n > 0] = it
    return last


class Case:
    def __init__(self, prob, lab64):
        self.N, self.H, self.W = (int(v) for v in prob.shape)
        self.prob, self.lab64 = prob.to(dev), lab64.to(dev)
        self.host = None

    def buffers(self, L):
        need = int(L.rsu_thin_ws_bytes(self.N, self.H, self.W, a.iters))
        return dict(sp=torch.zeros(self.prob.shape, dtype=torch.float32, device=dev), st=torch.zeros(self.prob.shape, dtype=torch.int64, device=dev),
                    acc=torch.zeros(4, dtype=torch.int64, device=dev), info=torch.zeros((self.N, 2), dtype=torch.int32, device=dev),
                    ws=torch.zeros(need // 8, dtype=torch.int64, device=dev), need=need)

    def thin_of(self, L, b):
        def run():
            b["acc"].zero_()
            rc = L.rsu_mask_thin(_ptr(self.prob), THR, _ptr(self.lab64), a.iters, _ptr(b["sp"]), _ptr(b["st"]), _ptr(b["acc"]), _ptr(b["info"]),
                                 _ptr(b["ws"]), self.N, self.H, self.W, st())
            assert rc == 0, rc
        return run

    def numpy_route(self):
        """what a user does today: copy to the host, the numpy restatement of the rule on both masks, both skeletons back"""
        p, y = self.prob.cpu().numpy(), self.lab64.cpu().numpy()
        sp, sy, counts, info = hostio.mask_thin(p, THR, y, a.iters)
        self.host = (sp, sy, counts, info)
        self.back = (torch.from_numpy(sp).to(dev), torch.from_numpy(sy).to(dev))


def timed(arms, rounds=20, slow=("copy + numpy restatement + copy",), slow_rounds=3):
    for name, fn in arms:
        for _ in range(1 if name in slow else 3):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k, _ in arms}
    for r in range(rounds):
        for name, fn in arms:
            if name in slow and r >= slow_rounds:
                continue
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(); us[name].append((time.perf_counter() - t0) * 1e6)
    return us


for S in (388, 608):
    for name, prob, lab64 in inputs(2, S):
        c = Case(prob, lab64)
        own = c.buffers(lib)
        print("N x H x W = 2 x %d x %d, %s; us per call between two synchronisations, median of 20 (min .. max)" % (S, S, name))
        arms = [("rsu_mask_thin (K = %d)" % OWN_K, c.thin_of(lib, own)), ("copy + numpy restatement + copy", c.numpy_route)]
        variants = [(k, L, c.buffers(L)) for k, L, _h in k_libs]
        arms += [("rsu_mask_thin, variant K = %d" % k, c.thin_of(L, b)) for k, L, b in variants]
        us = timed(arms)
        for arm, u in us.items():
            print("  %-38s %11.1f us (%.1f .. %.1f), %d calls" % (arm, median(u), min(u), max(u), len(u)))
        got = [own[k].cpu().numpy() for k in ("sp", "st", "acc", "info")]
        same_h = all(g.tobytes() == w.tobytes() for g, w in zip(got, (c.host[0], c.host[1], c.host[2], c.host[3].view(np.int32))))
        same_v = all(b[k].cpu().numpy().tobytes() == g.tobytes() for _k, _L, b in variants for k, g in zip(("sp", "st", "acc", "info"), got))
        tm, hm = median(us["rsu_mask_thin (K = %d)" % OWN_K]), median(us["copy + numpy restatement + copy"])
        print("  outputs equal the numpy restatement's byte for byte: %s; variants agree: %s; %.1f us against %.1f us: x %.0f"
              % (same_h, same_v, tm, hm, hm / tm))
        with np.errstate(invalid="ignore"):
            P, T = prob.numpy() >= np.float32(THR), lab64.numpy() == 1
        last = np.concatenate([last_deleting_iteration(P), last_deleting_iteration(T)])
        print("  skeleton pixels predicted %d true %d; last deleting iteration per image side %s; unconverged sides %d; workspace %d bytes"
              % (got[2][0], got[2][2], last.tolist(), int((got[3] != 0).sum()), own["need"]))
        for k in sorted({OWN_K} | {k for k, _L, _h in k_libs}):
            steps = -(-a.iters // k)
            work = [min(steps, 1 + -(-int(d) // k)) for d in last]
            print("  K = %d: %d launches per call (init + %d steps + final); step launches that return early: %d of %d image-side launches (%.0f %%)"
                  % (k, steps + 2, steps, sum(steps - w for w in work), steps * len(work), 100.0 * sum(steps - w for w in work) / (steps * len(work))))
