#!/usr/bin/env python3
"""Developer tool (GPU box): what the road-segment extraction on the device (include/rsu_segments.h) costs, and what it saves.

  bench_segments.py kernels
      rsu_line_segments (both tables, counts, the four maps and acc) at 2 x 388 x 388 and 2 x 608 x 608 against the only route a user
      has without it, on the same device tensors: device-to-host copy of the two skeletons, hostio.line_segments -- a NUMPY RESTATEMENT
      of the same definitions, not a library --, and the copy of the outputs back. Inputs: the pruned skeletons (rsu_mask_thin, 64
      iterations; rsu_skeleton_graph, min_branch 8) of a smooth road-like map (blurred noise through a sigmoid; the truth is the same map
      at a higher level). One process, the arms alternated call by call; every call is timed on the host between two synchronisations:
      us per call, median of 20 rounds with min and max (the numpy arm: 3 rounds).
  bench_segments.py split [--calls N] [--side S]
      N calls at 2 x S x S and nothing else: the process to put behind `rocprofv3 --kernel-trace --stats --` for the split by kernel.
  bench_segments.py step --lib PARENT_LIBRARY [--reps N]
      the DEFAULT config-2 training step and a DEFAULT validation pass (evaluate() over 8 patches of 388 x 388, no flag of this change
      set) with this tree's library against the parent commit's library (built as `make -C road_segmentation_unet_amd/csrc
      VARIANT=parent` in a checkout of the parent, loaded through RSU_LIB_PATH), alternating fresh processes on one box; the order of the
      arms rotates from round to round. Every process runs under its own time limit and the series stops at the first one that fails.
      Medians per arm; the spread of the parent arm's runs is the noise the difference is read against.
  bench_segments.py step --all-flags --lib PARENT_LIBRARY [--reps N]
      the same two arms per library, the validation pass with ALL FIVE mask stages on (below): for a change of the mask tools' kernels.
      The parent's library must then have every entry this tree's Python binds.
  bench_segments.py step --all-flags --parent-tree PARENT_CHECKOUT [--lib LIBRARY] [--reps N]
      a validation pass with ALL FIVE mask stages on (--validate_components, --validate_distances, --validate_centerlines with
      --centerline_min_branch=8, --validate_junctions and --validate_segments: evaluate() over the same 8 patches of 388 x 388 in chunks
      of 4), and the default pass again, with this tree's Python against a checkout of the parent commit's, both on ONE library (--lib,
      default this tree's): the same rotation of fresh processes. The verdict: this arm's median inside the parent arm's own min .. max,
      or below it.
  bench_segments.py arm [--validate [--all-flags] [--tree ROOT]] [--steps N]
      one arm of the above in this process. --parent-lib: the library is the parent commit's, which has no entry of rsu_segments.h --
      the table is left unbound (the default step and validation call none of them). --tree: the checkout whose package is imported.
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
ap.add_argument("mode_", metavar="mode", choices=["kernels", "split", "step", "arm"])
ap.add_argument("--lib", default=None)
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--reps", type=int, default=6)
ap.add_argument("--calls", type=int, default=50)
ap.add_argument("--side", type=int, default=608)
ap.add_argument("--validate", action="store_true")
ap.add_argument("--parent-lib", action="store_true")
ap.add_argument("--all-flags", action="store_true")
ap.add_argument("--parent-tree", default=None)
ap.add_argument("--tree", default=None)
a = ap.parse_args()


def median(v):
    return sorted(v)[len(v) // 2]


if a.mode_ == "step":
    if a.all_flags and (a.parent_tree or not a.lib):
        one_lib = os.path.abspath(a.lib or os.path.join(HERE, "road_segmentation_unet_amd", "librsu_hip.so"))
        if not a.parent_tree or not os.path.isdir(os.path.join(a.parent_tree, "road_segmentation_unet_amd")) or not os.path.exists(one_lib):
            sys.exit("step --all-flags needs --parent-tree: a checkout of the parent commit, and a built library")
        both, tree = {"RSU_LIB_PATH": one_lib}, ["--tree", os.path.abspath(a.parent_tree)]
        arms = [("parent all-flags", both, ["--validate", "--all-flags"] + tree), ("this all-flags", both, ["--validate", "--all-flags"]),
                ("parent default", both, ["--validate"] + tree), ("this default", both, ["--validate"])]
    else:
        if not a.lib or not os.path.exists(a.lib):
            sys.exit("step needs --lib: the parent commit's library")
        parent = {"RSU_LIB_PATH": os.path.abspath(a.lib)}
        old, val = ([], ["--validate", "--all-flags"]) if a.all_flags else (["--parent-lib"], ["--validate"])
        arms = [("parent step", parent, old), ("this step", {}, []), ("parent validate", parent, old + val), ("this validate", {}, val)]
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
    if a.all_flags and a.parent_tree:
        for what, title in (("all-flags", "all five mask stages on"), ("default", "no flag set")):
            lo, hi, this, par = min(ms["parent " + what]), max(ms["parent " + what]), med["this " + what], med["parent " + what]
            print("validation pass, %s, this tree's Python against the parent's on one library: median %.4f ms against %.4f ms (%+.2f %%); "
                  "the parent arm's own runs span %.4f .. %.4f ms: this median is %s"
                  % (title, this, par, 100 * (this - par) / par, lo, hi, "BELOW that range" if this < lo else "inside it" if this <= hi else "ABOVE it"))
        sys.exit(0)
    for what in ("step", "validate"):
        spread, own = max(ms["parent " + what]) - min(ms["parent " + what]), max(ms["this " + what]) - min(ms["this " + what])
        d = med["this " + what] - med["parent " + what]
        print("%s %s, this library - parent's (medians): %+.4f ms (%+.2f %%); run-to-run spread (max - min) of the parent arm %.4f ms, of "
              "this arm %.4f ms: %s the parent's" % ("all-flags" if a.all_flags and what == "validate" else "default", what, d,
                                                     100 * d / med["parent " + what], spread, own,
                                                     "inside" if abs(d) <= spread else "OUTSIDE"))
    sys.exit(0)

sys.path.insert(0, os.path.abspath(a.tree) if a.tree else HERE)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.nn.functional as Fn  # noqa: E402
from road_segmentation_unet_amd import _lib, hostio  # noqa: E402
from road_segmentation_unet_amd.unet import UNet, _ptr  # noqa: E402

if a.parent_lib:
    _lib.SIGNATURES_SEGMENTS.clear()
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

BRANCH_ALL = 8   # --centerline_min_branch of the all-flags arm

if a.mode_ == "arm":
    from road_segmentation_unet_amd.model import ConvolutionalModel, Options
    from road_segmentation_unet_amd.unet import input_size_needed
    stages = dict(validate_components=True, validate_distances=True, validate_centerlines=True, centerline_min_branch=BRANCH_ALL,
                  validate_junctions=True, validate_segments=True) if a.all_flags else {}
    opts = Options(num_layers=5, root_size=64, patch_size=388, batch_size=4, dropout=1.0, logdir=None, **stages)
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
    assert all((k in v) == a.all_flags for k in ("components_pred", "dist_hist", "cl_hist", "jn_hist", "segments_pred"))
    pkg = os.path.dirname(os.path.abspath(sys.modules[ConvolutionalModel.__module__].__file__))
    assert pkg == os.path.join(os.path.abspath(a.tree) if a.tree else HERE, "road_segmentation_unet_amd"), pkg
    print("%s validate lib %s, the package of %s, 8 patches of 388 x 388 in chunks of 4, 7 calls %s: %.4f ms/pass (median)"
          % ("all-flags" if a.all_flags else "default", sha, "the --tree checkout" if a.tree else "this tree", " ".join("%.1f" % x for x in t),
             median(t)))
    sys.exit(0)

# ---- kernels, split
print("lib %s, device %s" % (sha, torch.cuda.get_device_name(0)))
dev = "cuda:0"
lib = _lib.lib()
st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
THR, CAP, BRANCH = 0.5, 4096, 8


def inputs(N, S):
    """the two pruned skeletons of a smooth road-like map, thinned and pruned on the device: (skel_pred float32, skel_true int64)"""
    gen = torch.Generator(device="cpu").manual_seed(1)
    noise = torch.randn((N, 1, S, S), generator=gen)
    for _ in range(6):
        noise = Fn.avg_pool2d(noise, 5, 1, 2)
    smooth = torch.sigmoid(noise[:, 0] / noise.std() * 3.0 - 1.0).contiguous()
    p, y = smooth.to(dev), (smooth >= 0.6).to(torch.int64).to(dev)
    sp, sy = torch.zeros_like(p), torch.zeros_like(y)
    ws = torch.zeros(int(lib.rsu_thin_ws_bytes(N, S, S, 64)) // 8, dtype=torch.int64, device=dev)
    rc = lib.rsu_mask_thin(_ptr(p), THR, _ptr(y), 64, _ptr(sp), _ptr(sy), None, None, _ptr(ws), N, S, S, st())
    assert rc == 0, rc
    ws = torch.zeros(int(lib.rsu_graph_ws_bytes(N, S, S, BRANCH)) // 8, dtype=torch.int64, device=dev)
    rc = lib.rsu_skeleton_graph(_ptr(sp), THR, _ptr(sy), BRANCH, _ptr(sp), _ptr(sy), None, None, None, _ptr(ws), N, S, S, st())
    assert rc == 0, rc
    return sp, sy


KEYS = ("ep", "et", "counts", "sp", "st", "np", "nt", "acc")


class Case:
    def __init__(self, sp, sy):
        self.N, self.H, self.W = (int(v) for v in sp.shape)
        self.sp, self.sy = sp, sy
        self.host = None

    def buffers(self, L):
        need = int(L.rsu_segments_ws_bytes(self.N, self.H, self.W, CAP))
        table = lambda: torch.zeros((self.N, CAP, 8), dtype=torch.int32, device=dev)   # noqa: E731
        plane = lambda: torch.zeros(self.sp.shape, dtype=torch.int32, device=dev)      # noqa: E731
        return {"ep": table(), "et": table(), "counts": torch.zeros((self.N, 4), dtype=torch.int32, device=dev), "sp": plane(), "st": plane(),
                "np": plane(), "nt": plane(), "acc": torch.zeros((2, 8), dtype=torch.int64, device=dev),
                "ws": torch.zeros(need // 8, dtype=torch.int64, device=dev), "need": need}

    def segments_of(self, L, buf):
        def run():
            buf["acc"].zero_()
            rc = L.rsu_line_segments(_ptr(self.sp), THR, _ptr(self.sy), CAP, _ptr(buf["ep"]), _ptr(buf["et"]), _ptr(buf["counts"]), _ptr(buf["sp"]),
                                     _ptr(buf["st"]), _ptr(buf["np"]), _ptr(buf["nt"]), _ptr(buf["acc"]), _ptr(buf["ws"]), self.N, self.H, self.W, st())
            assert rc == 0, rc
        return run

    def numpy_route(self):
        """what a user does today: copy to the host, the numpy restatement of the definitions on both masks, the outputs back"""
        def run():
            p, y = self.sp.cpu().numpy(), self.sy.cpu().numpy()
            self.host = hostio.line_segments(p, THR, y, CAP)
            self.back = [torch.from_numpy(x).to(dev) for x in self.host]
        return run


if a.mode_ == "split":
    S = a.side
    c = Case(*inputs(2, S))
    buf = c.buffers(lib)
    run = c.segments_of(lib, buf)
    for _ in range(a.calls):
        run()
    torch.cuda.synchronize()
    print("%d calls of rsu_line_segments at 2 x %d x %d, max_edges %d; counts %s" % (a.calls, S, S, CAP, buf["counts"].cpu().numpy().tolist()))
    sys.exit(0)


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


for S in (388, 608):
    c = Case(*inputs(2, S))
    own = c.buffers(lib)
    print("N x H x W = 2 x %d x %d, max_edges %d, pruned (min_branch %d) skeletons of a smooth road-like map (truth: the map >= 0.6); us per "
          "call between two synchronisations, median of 20 (min .. max)" % (S, S, CAP, BRANCH))
    arms = [("rsu_line_segments", c.segments_of(lib, own)), ("copy + numpy restatement + copy", c.numpy_route())]
    us = timed(arms)
    for arm, u in us.items():
        print("  %-40s %11.1f us (%.1f .. %.1f), %d calls" % (arm, median(u), min(u), max(u), len(u)))
    got = [own[k].cpu().numpy() for k in KEYS]
    counts = got[2]
    same_h = all(g.tobytes() == w.tobytes() for g, w in zip(got, c.host))   # (rows past the count: zeros on both sides)
    tm, hm = median(us["rsu_line_segments"]), median(us["copy + numpy restatement + copy"])
    print("  outputs equal the numpy restatement's byte for byte: %s; %.1f us against %.1f us: x %.0f" % (same_h, tm, hm, hm / tm))
    print("  counts {segments P, nodes P, segments T, nodes T} per image %s; acc %s; workspace %d bytes" % (counts.tolist(), got[7].tolist(), own["need"]))
    print("  ", {k: (round(v, 2) if isinstance(v, float) else v) for k, v in hostio.segment_metrics(got[7], counts.sum(axis=0).astype(np.int64)).items()})
