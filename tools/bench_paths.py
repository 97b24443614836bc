#!/usr/bin/env python3
"""Developer tool (GPU box): what the ordering of segment pixels on the device (include/rsu_paths.h) costs, and what it saves.

  bench_paths.py kernels
      rsu_segment_paths (paths, offsets, kind, pos and info of the prediction's side, max_len 4096, max_points H W) at 2 x 388 x 388 and
      2 x 608 x 608 against the only route a user has without it, on the same device tensors: device-to-host copy of seg, edges and
      counts, hostio.segment_paths -- a sequential walk in Python, a RESTATEMENT of the same definitions, not a library --, and the copy
      of the outputs back. Inputs: rsu_line_segments of the pruned skeletons (rsu_mask_thin, 64 iterations; rsu_skeleton_graph,
      min_branch 8) of a smooth road-like map (blurred noise through a sigmoid). One process, the arms alternated call by call; every
      call is timed on the host between two synchronisations: us per call, median of 20 rounds with min and max (the host arm: 3 rounds).
      Then, per image, the changed-arc counts of every jump launch, read from the workspace: how many doublings an image needs and how
      many launches return early for it.
  bench_paths.py split [--calls N] [--side S]
      N calls at 2 x S x S and nothing else: the process to put behind `rocprofv3 --kernel-trace --stats --` for the split by kernel.
  bench_paths.py graph
      ConvolutionalModel.road_graph() end to end on 2 masks of 388 x 388 and of 608 x 608 with --road_graph_paths against without, one
      process, the arms alternated: ms per call, median of 7.
  bench_paths.py step --lib PARENT_LIBRARY [--reps N]
      the DEFAULT config-2 training step and a DEFAULT validation pass (evaluate() over 8 patches of 388 x 388, no flag of this change
      set) with this tree's library against the parent commit's library (built as `make -C road_segmentation_unet_amd/csrc
      VARIANT=parent` in a checkout of the parent, loaded through RSU_LIB_PATH), alternating fresh processes on one box; the order of the
      arms rotates from round to round. Every process runs under its own time limit and the series stops at the first one that fails.
      Medians per arm; the spread of the parent arm's runs is the noise the difference is read against.
  bench_paths.py arm [--validate] [--parent-lib] [--steps N]
      one arm of the above in this process. --parent-lib: the library is the parent commit's, which has no entry of rsu_paths.h -- the
      table is left unbound (the default step and validation call none of them).
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
ap.add_argument("mode_", metavar="mode", choices=["kernels", "split", "graph", "step", "arm"])
ap.add_argument("--lib", default=None)
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--reps", type=int, default=6)
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--side", type=int, default=608)
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
    _lib.SIGNATURES_PATHS.clear()
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
    model = ConvolutionalModel(Options(num_layers=5, root_size=64, patch_size=388, batch_size=4, dropout=1.0, logdir=None))
    rng = np.random.RandomState(0)
    S = input_size_needed(388, 5)
    X, y = rng.rand(8, S, S, 3).astype(np.float32), (rng.rand(8, 388, 388) < 0.2).astype(np.int64)
    model.evaluate(X, y)
    model.evaluate(X, y)
    t = []
    for _ in range(7):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        model.evaluate(X, y)
        torch.cuda.synchronize(); t.append((time.perf_counter() - t0) * 1e3)
    print("default validate lib %s, 8 patches of 388 x 388 in chunks of 4, 7 calls %s: %.4f ms/pass (median)"
          % (sha, " ".join("%.1f" % x for x in t), median(t)))
    sys.exit(0)

print("lib %s, device %s" % (sha, torch.cuda.get_device_name(0)))
dev = "cuda:0"
lib = _lib.lib()
st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
THR, CAP, BRANCH, MAX_LEN = 0.5, 4096, 8, 4096


def smooth_map(N, S):
    gen = torch.Generator(device="cpu").manual_seed(1)
    noise = torch.randn((N, 1, S, S), generator=gen)
    for _ in range(6):
        noise = Fn.avg_pool2d(noise, 5, 1, 2)
    return torch.sigmoid(noise[:, 0] / noise.std() * 3.0 - 1.0).contiguous()


if a.mode_ == "graph":
    from road_segmentation_unet_amd.model import ConvolutionalModel, Options
    models = {flag: ConvolutionalModel(Options(num_layers=2, root_size=16, patch_size=16, batch_size=4, dropout=1.0, logdir=None,
                                               centerline_min_branch=BRANCH, road_graph_paths=flag)) for flag in (False, True)}
    for S in (388, 608):
        masks = smooth_map(2, S).numpy()
        ms = {False: [], True: []}
        for r in range(9):
            for flag in (False, True):
                torch.cuda.synchronize(); t0 = time.perf_counter()
                g = models[flag].road_graph(masks, threshold=THR)
                torch.cuda.synchronize()
                if r >= 2:
                    ms[flag].append((time.perf_counter() - t0) * 1e3)
                if flag:
                    points, unordered, edges = sum(len(e["path"]) for q in g for e in q["edges"]), sum(q["unordered"] for q in g), sum(len(q["edges"]) for q in g)
        print("road_graph() of 2 masks of %d x %d, min_branch %d, ms per call, median of 7 (min .. max): without --road_graph_paths %.1f "
              "(%.1f .. %.1f), with %.1f (%.1f .. %.1f); %d edges, %d path points, %d segments not ordered"
              % (S, S, BRANCH, median(ms[False]), min(ms[False]), max(ms[False]), median(ms[True]), min(ms[True]), max(ms[True]), edges, points,
                 unordered))
    sys.exit(0)


class Case:
    """the inputs of rsu_segment_paths from rsu_line_segments of the pruned skeleton of a smooth road-like map, and the entry's buffers"""

    def __init__(self, N, S):
        self.N, self.H, self.W = N, S, S
        p = smooth_map(N, S).to(dev)
        sp = torch.zeros_like(p)
        ws = torch.zeros(int(lib.rsu_thin_ws_bytes(N, S, S, 64)) // 8, dtype=torch.int64, device=dev)
        assert lib.rsu_mask_thin(_ptr(p), THR, None, 64, _ptr(sp), None, None, None, _ptr(ws), N, S, S, st()) == 0
        ws = torch.zeros(int(lib.rsu_graph_ws_bytes(N, S, S, BRANCH)) // 8, dtype=torch.int64, device=dev)
        assert lib.rsu_skeleton_graph(_ptr(sp), THR, None, BRANCH, _ptr(sp), None, None, None, None, _ptr(ws), N, S, S, st()) == 0
        z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)   # noqa: E731
        self.seg, self.edges, self.counts = z(N, S, S), z(N, CAP, 8), z(N, 4)
        ws = torch.zeros(int(lib.rsu_segments_ws_bytes(N, S, S, CAP)) // 8, dtype=torch.int64, device=dev)
        assert lib.rsu_line_segments(_ptr(sp), THR, None, CAP, _ptr(self.edges), None, _ptr(self.counts), _ptr(self.seg), None, None, None, None,
                                     _ptr(ws), N, S, S, st()) == 0
        self.need = int(lib.rsu_paths_ws_bytes(N, S, S, CAP, MAX_LEN))
        self.ws = torch.zeros(self.need // 8, dtype=torch.int64, device=dev)
        self.out = [z(N, S * S), z(N, CAP + 1), z(N, CAP), z(N, S, S), z(N, 4)]
        self.host = None

    def entry(self):
        rc = lib.rsu_segment_paths(_ptr(self.seg), _ptr(self.edges), _ptr(self.counts), 0, CAP, MAX_LEN, self.H * self.W, *(_ptr(t) for t in self.out),
                                   _ptr(self.ws), self.N, self.H, self.W, st())
        assert rc == 0, rc

    def host_route(self):
        """what a user does today: copy to the host, walk every segment in Python, the outputs back"""
        seg, edges, counts = self.seg.cpu().numpy(), self.edges.cpu().numpy(), self.counts.cpu().numpy()
        self.host = hostio.segment_paths(seg, edges, counts, 0, MAX_LEN, self.H * self.W)
        self.back = [torch.from_numpy(x).to(dev) for x in self.host]

    def jump_counts(self):
        """int [R][N]: the changed arcs of every jump launch, the last array of the workspace"""
        R = hostio.path_rounds(MAX_LEN)
        px = self.N * self.H * self.W
        at = px * 36 + 2 * self.N * CAP * 4
        return self.ws.view(torch.int32)[at // 4:at // 4 + R * self.N].reshape(R, self.N).cpu().numpy()


if a.mode_ == "split":
    c = Case(2, a.side)
    for _ in range(a.calls):
        c.entry()
    torch.cuda.synchronize()
    print("%d calls of rsu_segment_paths at 2 x %d x %d, max_edges %d, max_len %d (%d launches each); info %s"
          % (a.calls, a.side, a.side, CAP, MAX_LEN, 5 + hostio.path_rounds(MAX_LEN), c.out[4].cpu().numpy().tolist()))
    sys.exit(0)

SLOW = "copy + sequential walk on the host + copy"
for S in (388, 608):
    c = Case(2, S)
    arms = [("rsu_segment_paths", c.entry), (SLOW, c.host_route)]
    for name, fn in arms:
        for _ in range(1 if name == SLOW else 3):
            fn()
    torch.cuda.synchronize()
    us = {k: [] for k, _ in arms}
    for r in range(20):
        for name, fn in arms:
            if name == SLOW and r >= 3:
                continue
            torch.cuda.synchronize(); t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(); us[name].append((time.perf_counter() - t0) * 1e6)
    print("N x H x W = 2 x %d x %d, max_edges %d, max_len %d, the prediction's side of rsu_line_segments on the pruned (min_branch %d) skeletons "
          "of a smooth road-like map; us per call between two synchronisations, median of 20 (min .. max)" % (S, S, CAP, MAX_LEN, BRANCH))
    for arm, u in us.items():
        print("  %-45s %11.1f us (%.1f .. %.1f), %d calls" % (arm, median(u), min(u), max(u), len(u)))
    got = [t.cpu().numpy() for t in c.out]
    same = all(g.tobytes() == w.tobytes() for g, w in zip(got, c.host))   # (untouched elements: zeros on both sides)
    tm, hm = median(us["rsu_segment_paths"]), median(us[SLOW])
    print("  outputs equal the host walk's byte for byte: %s; %.1f us against %.1f us: x %.0f" % (same, tm, hm, hm / tm))
    info, kind = got[4], got[2]
    longest = [int(c.edges[n, :min(int(c.counts[n, 0]), CAP), 1].max()) for n in range(2)]
    print("  info {points, open, ring, unordered} per image %s; the longest segment per image %s pixels; workspace %d bytes; %d launches"
          % (info.tolist(), longest, c.need, 5 + hostio.path_rounds(MAX_LEN)))
    jc = c.jump_counts()
    print("  changed arcs per jump launch and image: %s" % jc.tolist())
    print("  jump launches that return early (the count of the launch before is 0), per image: %s of %d"
          % ([int(sum(1 for r in range(1, jc.shape[0]) if jc[r - 1, n] == 0)) for n in range(2)], jc.shape[0]))
