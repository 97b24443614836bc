#!/usr/bin/env python3
"""Developer tool (GPU box): what the centre-line pruning and node classification on the device (include/rsu_graph.h) costs, and what it
saves.

  bench_graph.py kernels [--r-libs R=LIBRARY,R=LIBRARY,...]
      rsu_skeleton_graph (all four outputs and acc) at 2 x 388 x 388 and 2 x 608 x 608 and min_branch 0, 8 and 64 against the only route
      a user has without it, on the same device tensors: device-to-host copy of the two skeletons, hostio.skeleton_graph -- a NUMPY
      RESTATEMENT of the same rule, not a library: no library pruning is installed -- and the copy of the four outputs back. Inputs: the
      skeletons (rsu_mask_thin, 64 iterations) of a smooth road-like map (blurred noise through a sigmoid; the truth is the same map at a
      higher level) and of the test bank's random masks (rand0.55 against rand0.45). One process, the arms alternated call by call; every
      call is timed on the host between two synchronisations: us per call, median of 20 rounds with min and max (the numpy arm: 3
      rounds). --r-libs: A/B builds of the library that differ in the rounds a step launch carries
      (make -C road_segmentation_unet_amd/csrc VARIANT=graphR EXTRA=-DGR_R=R); each is timed in the same alternation with a workspace of
      its own size, and every arm's outputs must equal the first's. For every R the share of step launches that return early is derived
      from the round at which each image side stops changing (counted on the host).
  bench_graph.py step --lib PARENT_LIBRARY [--reps N]
      the DEFAULT config-2 training step and a DEFAULT validation pass (evaluate() over 8 patches of 388 x 388, no flag of this change
      set) with this tree's library against the parent commit's library (built as `make -C road_segmentation_unet_amd/csrc
      VARIANT=parent` in a checkout of the parent, loaded through RSU_LIB_PATH), alternating fresh processes on one box; the order of the
      arms rotates from round to round. Every process runs under its own time limit and the series stops at the first one that fails.
      Medians per arm; the spread of the parent arm's runs is the noise the difference is read against.
  bench_graph.py arm [--validate] [--steps N]
      one arm of the above in this process. --parent-lib: the library is the parent commit's, which has no entry of rsu_graph.h -- the
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
ap.add_argument("--r-libs", default="")
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
    _lib.SIGNATURES_GRAPH.clear()
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
    assert "cl_hist" not in v and "jn_hist" not in v
    print("default validate lib %s, 8 patches of 388 x 388 in chunks of 4, 7 calls %s: %.4f ms/pass (median)"
          % (sha, " ".join("%.1f" % x for x in t), median(t)))
    sys.exit(0)

# ---- kernels
print("lib %s, device %s" % (sha, torch.cuda.get_device_name(0)))
dev = "cuda:0"
lib = _lib.lib()
st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
THR = 0.5
BRANCHES = (0, 8, 64)
src = open(os.path.join(HERE, "road_segmentation_unet_amd", "csrc", "graph.h")).read()
OWN_R = int(re.search(r"^#define GR_R (\d+)$", src, flags=re.M).group(1))
r_libs = []
for item in [s for s in a.r_libs.split(",") if s]:
    k, path = item.split("=", 1)
    L = ctypes.CDLL(os.path.abspath(path))
    for name in _lib.SIGNATURES_GRAPH:
        getattr(L, name).restype, getattr(L, name).argtypes = _lib.SIGNATURES_GRAPH[name]
    r_libs.append((int(k), L, hashlib.sha256(open(path, "rb").read()).hexdigest()[:16]))
for k, _L, h in r_libs:
    print("variant: %d round(s) per step launch, lib %s" % (k, h))


def inputs(N, S):
    """the two skeletons of each input pair, thinned on the device: (name, skel_pred float32, skel_true int64)"""
    gen = torch.Generator(device="cpu").manual_seed(1)
    noise = torch.randn((N, 1, S, S), generator=gen)
    for _ in range(6):
        noise = Fn.avg_pool2d(noise, 5, 1, 2)
    smooth = torch.sigmoid(noise[:, 0] / noise.std() * 3.0 - 1.0).contiguous()
    rs = np.random.RandomState(7)
    rnd = torch.from_numpy(np.where(rs.random_sample((N, S, S)) < 0.55, 0.75, 0.25).astype(np.float32))
    rnd_true = torch.from_numpy((rs.random_sample((N, S, S)) < 0.45).astype(np.int64))
    out = []
    for name, prob, lab in (("thinned smooth road-like map (truth: the map >= 0.6)", smooth, (smooth >= 0.6).to(torch.int64)),
                            ("the test bank's random masks, thinned (rand0.55 against rand0.45)", rnd, rnd_true)):
        p, y = prob.to(dev), lab.to(dev)
        sp, sy = torch.zeros_like(p), torch.zeros_like(y)
        ws = torch.zeros(int(lib.rsu_thin_ws_bytes(N, S, S, 64)) // 8, dtype=torch.int64, device=dev)
        rc = lib.rsu_mask_thin(_ptr(p), THR, _ptr(y), 64, _ptr(sp), _ptr(sy), None, None, _ptr(ws), N, S, S, st())
        assert rc == 0, rc
        out.append((name, sp, sy))
    return out


def stop_rounds(mask, L):
    """per image: (the last delete round that deletes a pixel, the last regrow round that adds one) of hostio.prune_mask at L"""
    x1 = mask.copy()
    dele = np.zeros(mask.shape[0], np.int64)
    for r in range(1, L + 1):
        d = hostio._graph_end(x1)
        dele[d.reshape(d.shape[0], -1).any(axis=1)] = r
        x1 &= ~d
    e = hostio._graph_end(x1)
    grow = np.zeros(mask.shape[0], np.int64)
    H, W = mask.shape[1:]
    for r in range(1, L + 1):
        q = np.pad(e, ((0, 0), (1, 1), (1, 1)))
        d = np.zeros_like(e)
        for dy in (0, 1, 2):
            for dx in (0, 1, 2):
                d |= q[:, dy:dy + H, dx:dx + W]
        n = mask & d
        grow[(n & ~e).reshape(n.shape[0], -1).any(axis=1)] = r
        e = n
    return dele, grow, e.reshape(e.shape[0], -1).any(axis=1)


def early_share(dele, grow, any_end, L, R):
    """(step launches that return early, step launches) over the image sides: delete launch s works iff s == 0 or launch s - 1 deleted
    a pixel; regrow launch 0 works iff the last delete launch did, launch g iff launch g - 1 added a pixel"""
    D, G = -(-L // R), -(-(L + 1) // R)
    early = total = 0
    for d, g, e in zip(dele, grow, any_end):
        total += D + G
        ran = [True] + [d > (s - 1) * R for s in range(1, D)]
        last_deleted = ran[-1] and d > (D - 1) * R
        first = R - 1
        rr = [last_deleted]
        for k in range(1, G):
            lo = 0 if k == 1 else first + (k - 2) * R
            rr.append(rr[-1] and ((e and k == 1) or g > lo))
        early += sum(not v for v in ran) + sum(not v for v in rr)
    return early, total


class Case:
    def __init__(self, sp, sy):
        self.N, self.H, self.W = (int(v) for v in sp.shape)
        self.sp, self.sy = sp, sy
        self.host = {}

    def buffers(self, L, b):
        need = int(L.rsu_graph_ws_bytes(self.N, self.H, self.W, b))
        f, i = (lambda: torch.zeros(self.sp.shape, dtype=torch.float32, device=dev)), (lambda: torch.zeros(self.sp.shape, dtype=torch.int64, device=dev))
        return dict(op=f(), ot=i(), jp=f(), jt=i(), acc=torch.zeros(8, dtype=torch.int64, device=dev),
                    ws=torch.zeros(need // 8, dtype=torch.int64, device=dev), need=need)

    def graph_of(self, L, buf, b):
        def run():
            buf["acc"].zero_()
            rc = L.rsu_skeleton_graph(_ptr(self.sp), THR, _ptr(self.sy), b, _ptr(buf["op"]), _ptr(buf["ot"]), _ptr(buf["jp"]), _ptr(buf["jt"]),
                                      _ptr(buf["acc"]), _ptr(buf["ws"]), self.N, self.H, self.W, st())
            assert rc == 0, rc
        return run

    def numpy_route(self, b):
        """what a user does today: copy to the host, the numpy restatement of the rule on both masks, the four outputs back"""
        def run():
            p, y = self.sp.cpu().numpy(), self.sy.cpu().numpy()
            self.host[b] = hostio.skeleton_graph(p, THR, y, b)
            self.back = [torch.from_numpy(x).to(dev) for x in self.host[b][:4]]
        return run


def timed(arms, rounds=20, slow="copy + numpy restatement + copy", slow_rounds=3):
    for name, fn in arms:
        for _ in range(1 if name == slow else 3):
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


KEYS = ("op", "ot", "jp", "jt", "acc")
for S in (388, 608):
    for name, sp, sy in inputs(2, S):
        c = Case(sp, sy)
        masks = (sp.cpu().numpy() >= np.float32(THR), sy.cpu().numpy() == 1)
        for b in BRANCHES:
            own = c.buffers(lib, b)
            print("N x H x W = 2 x %d x %d, min_branch %d, %s; us per call between two synchronisations, median of 20 (min .. max)" % (S, S, b, name))
            own_name = "rsu_skeleton_graph (R = %d)" % OWN_R
            arms = [(own_name, c.graph_of(lib, own, b)), ("copy + numpy restatement + copy", c.numpy_route(b))]
            variants = [(k, L, c.buffers(L, b)) for k, L, _h in r_libs]
            arms += [("rsu_skeleton_graph, variant R = %d" % k, c.graph_of(L, buf, b)) for k, L, buf in variants]
            us = timed(arms)
            for arm, u in us.items():
                print("  %-38s %11.1f us (%.1f .. %.1f), %d calls" % (arm, median(u), min(u), max(u), len(u)))
            got = [own[k].cpu().numpy() for k in KEYS]
            same_h = all(g.tobytes() == w.tobytes() for g, w in zip(got, c.host[b]))
            same_v = all(buf[k].cpu().numpy().tobytes() == g.tobytes() for _k, _L, buf in variants for k, g in zip(KEYS, got))
            tm, hm = median(us[own_name]), median(us["copy + numpy restatement + copy"])
            print("  outputs equal the numpy restatement's byte for byte: %s; variants agree: %s; %.1f us against %.1f us: x %.0f"
                  % (same_h, same_v, tm, hm, hm / tm))
            print("  {|B|, ends, isolated, junction pixels} predicted %s true %s; workspace %d bytes" % (got[4][:4].tolist(), got[4][4:].tolist(), own["need"]))
            if b:
                stops = [stop_rounds(m, b) for m in masks]
                dele, grow, any_end = (np.concatenate([s[i] for s in stops]) for i in range(3))
                print("  last deleting round per image side %s, last growing round %s" % (dele.tolist(), grow.tolist()))
                for k in sorted({OWN_R} | {k for k, _L, _h in r_libs}):
                    early, total = early_share(dele, grow, any_end, b, k)
                    print("  R = %d: %d launches per call (init + %d delete + %d regrow + final); step launches that return early: %d of %d "
                          "image-side launches (%.0f %%)" % (k, 2 + -(-b // k) + -(-(b + 1) // k), -(-b // k), -(-(b + 1) // k), early, total,
                                                             100.0 * early / total))
