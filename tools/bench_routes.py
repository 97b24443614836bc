#!/usr/bin/env python3
"""Developer tool (GPU box): what the network distances and the path-length score on the device (include/rsu_routes.h) cost, and what
they save.

  bench_routes.py kernels
      rsu_graph_routes of both sides and rsu_route_score in both directions (max_nodes 1024, snap 8) at 2 x 388 x 388 and 2 x 608 x 608
      against the route a user has without them, on the same device tensors: device-to-host copy of the node maps, the rows and counts,
      the node table and weights of hostio.graph_routes with scipy.sparse.csgraph.shortest_path per image and side in place of its
      Floyd-Warshall loop, hostio.route_score's matching and pairs, and the copy of the outputs back. Inputs: rsu_line_segments of the
      pruned skeletons (rsu_mask_thin, 64 iterations; rsu_skeleton_graph, min_branch 8) of two smooth road-like maps (blurred noise
      through a sigmoid; the truth is another seed). One process, the arms alternated call by call; every call is timed on the host
      between two synchronisations: us per call, median of 20 rounds with min and max (the host arm: 3 rounds). Then how many of the
      Floyd-Warshall launches return at once for every image.
  bench_routes.py split [--calls N] [--side S]
      N calls of the device arm at 2 x S x S and nothing else: the process to put behind `rocprofv3 --kernel-trace --stats --` for the
      split by kernel.
  bench_routes.py flags
      evaluate() over 8 patches of 388 x 388 with every mask flag on, with and without --validate_routes, one process, the arms
      alternated: ms per pass, median of 7.
  bench_routes.py step --lib PARENT_LIBRARY [--reps N]
      the DEFAULT config-2 training step and a DEFAULT validation pass (evaluate() over 8 patches of 388 x 388, no flag of this change
      set) with this tree's library against the parent commit's library (loaded through RSU_LIB_PATH), alternating fresh processes on
      one box; the order of the arms rotates from round to round. Every process runs under its own time limit and the series stops at
      the first one that fails. Medians per arm; the spread of the parent arm's runs is the noise the difference is read against.
  bench_routes.py arm [--validate] [--parent-lib] [--steps N]
      one arm of the above in this process. --parent-lib: the library is the parent commit's, which has no entry of rsu_routes.h -- the
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
ap.add_argument("mode_", metavar="mode", choices=["kernels", "split", "flags", "step", "arm"])
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
    _lib.ROUTES_SIGNATURES.clear()
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


def evaluate_ms(**flags):
    from road_segmentation_unet_amd.model import ConvolutionalModel, Options
    from road_segmentation_unet_amd.unet import input_size_needed
    model = ConvolutionalModel(Options(num_layers=5, root_size=64, patch_size=388, batch_size=4, dropout=1.0, logdir=None, **flags))
    rng = np.random.RandomState(0)
    S = input_size_needed(388, 5)
    X, y = rng.rand(8, S, S, 3).astype(np.float32), (rng.rand(8, 388, 388) < 0.2).astype(np.int64)
    return model, X, y


if a.mode_ == "arm":
    model, X, y = evaluate_ms()
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

if a.mode_ == "flags":
    on = dict(validate_components=True, validate_distances=True, validate_centerlines=True, centerline_min_branch=8, validate_junctions=True,
              validate_segments=True)
    models = {flag: evaluate_ms(validate_routes=flag, **on) for flag in (False, True)}
    ms = {False: [], True: []}
    for r in range(9):
        for flag in (False, True):
            model, X, y = models[flag]
            torch.cuda.synchronize(); t0 = time.perf_counter()
            v = model.evaluate(X, y)
            torch.cuda.synchronize()
            if r >= 2:
                ms[flag].append((time.perf_counter() - t0) * 1e3)
            if flag:
                keys = {k: v[k] for k in ("apls", "route_pairs_true_to_pred", "route_pairs_pred_to_true", "graph_nodes_pred", "graph_nodes_true",
                                          "graph_nodes_dropped_pred", "graph_nodes_dropped_true")}
    print("evaluate() over 8 patches of 388 x 388 (random labels, an untrained net), every mask flag on, min_branch 8, ms per pass, median of 7 "
          "(min .. max): without --validate_routes %.1f (%.1f .. %.1f), with %.1f (%.1f .. %.1f); %s"
          % (median(ms[False]), min(ms[False]), max(ms[False]), median(ms[True]), min(ms[True]), max(ms[True]), keys))
    sys.exit(0)

dev = "cuda:0"
lib = _lib.lib()
st = lambda: torch.cuda.current_stream().cuda_stream  # noqa: E731
THR, CAP, BRANCH, MAX_NODES, SNAP = 0.5, 4096, 8, 1024, 8


def smooth_map(N, S, seed):
    gen = torch.Generator(device="cpu").manual_seed(seed)
    noise = torch.randn((N, 1, S, S), generator=gen)
    for _ in range(6):
        noise = Fn.avg_pool2d(noise, 5, 1, 2)
    return torch.sigmoid(noise[:, 0] / noise.std() * 3.0 - 1.0).contiguous()


def scipy_solver(D):
    from scipy.sparse import csr_matrix
    from scipy.sparse.csgraph import shortest_path
    k = D.shape[0]
    if k == 0:
        return D
    i, j = np.nonzero((D < hostio.ROUTES_INF) & ~np.eye(k, dtype=bool))
    g = csr_matrix((D[i, j].astype(np.float64) + 0.25 / k, (i, j)), shape=(k, k))   # (+ 1 / (4 k): a zero weight stays an edge)
    d = shortest_path(g, method="auto", directed=False)
    out = np.where(np.isfinite(d), np.floor(np.where(np.isfinite(d), d, 0.0)), hostio.ROUTES_INF).astype(np.int64)
    out[np.arange(k), np.arange(k)] = 0
    return np.minimum(out, hostio.ROUTES_INF).astype(np.int32)


class Case:
    """the inputs of rsu_graph_routes from rsu_line_segments of the pruned skeletons of two smooth road-like maps, and the entries' buffers"""

    def __init__(self, N, S):
        self.N, self.H, self.W = N, S, S
        p = smooth_map(N, S, 1).to(dev)
        lab = (smooth_map(N, S, 2) >= THR).to(torch.int64).to(dev)
        sp, sl = torch.zeros_like(p), torch.zeros_like(lab)
        ws = torch.zeros(int(lib.rsu_thin_ws_bytes(N, S, S, 64)) // 8, dtype=torch.int64, device=dev)
        assert lib.rsu_mask_thin(_ptr(p), THR, _ptr(lab), 64, _ptr(sp), _ptr(sl), None, None, _ptr(ws), N, S, S, st()) == 0
        ws = torch.zeros(int(lib.rsu_graph_ws_bytes(N, S, S, BRANCH)) // 8, dtype=torch.int64, device=dev)
        assert lib.rsu_skeleton_graph(_ptr(sp), THR, _ptr(sl), BRANCH, _ptr(sp), _ptr(sl), None, None, None, _ptr(ws), N, S, S, st()) == 0
        z = lambda *shape: torch.zeros(shape, dtype=torch.int32, device=dev)   # noqa: E731
        self.maps, self.edges, self.counts = [z(N, S, S), z(N, S, S)], [z(N, CAP, 8), z(N, CAP, 8)], z(N, 4)
        ws = torch.zeros(int(lib.rsu_segments_ws_bytes(N, S, S, CAP)) // 8, dtype=torch.int64, device=dev)
        assert lib.rsu_line_segments(_ptr(sp), THR, _ptr(sl), CAP, _ptr(self.edges[0]), _ptr(self.edges[1]), _ptr(self.counts), None, None,
                                     _ptr(self.maps[0]), _ptr(self.maps[1]), None, _ptr(ws), N, S, S, st()) == 0
        self.need = int(lib.rsu_routes_ws_bytes(N, S, S, MAX_NODES))
        self.ws = torch.zeros(self.need // 4, dtype=torch.int32, device=dev)
        self.g = [[z(N, MAX_NODES, 4), z(N, MAX_NODES, MAX_NODES), z(N, 4)] for _ in (0, 1)]
        self.match = [z(N, MAX_NODES), z(N, MAX_NODES)]
        self.acc = torch.zeros((2, 4), dtype=torch.int64, device=dev)
        self.host = None

    def entries(self):
        self.acc.zero_()
        for side in (0, 1):
            rc = lib.rsu_graph_routes(_ptr(self.maps[side]), _ptr(self.edges[side]), _ptr(self.counts), side, CAP, MAX_NODES,
                                      *(_ptr(t) for t in self.g[side]), _ptr(self.ws), self.N, self.H, self.W, st())
            assert rc == 0, rc
        for d in (0, 1):   # truth -> prediction, then back
            x, y = self.g[1 - d], self.g[d]
            rc = lib.rsu_route_score(*(_ptr(t) for t in x), *(_ptr(t) for t in y), MAX_NODES, SNAP, _ptr(self.match[d]), _ptr(self.acc[d]), self.N, st())
            assert rc == 0, rc

    def host_route(self):
        """what a user does today: copy to the host, scipy's shortest paths per image and side, the matching and the pairs in numpy, back"""
        counts = self.counts.cpu().numpy()
        g = [hostio.graph_routes(self.maps[s].cpu().numpy(), self.edges[s].cpu().numpy(), counts, s, MAX_NODES, solver=scipy_solver) for s in (0, 1)]
        score = [hostio.route_score(*g[1 - d], *g[d], SNAP) for d in (0, 1)]
        self.host = (g, score)
        self.back = [torch.from_numpy(x).to(dev) for s in (0, 1) for x in g[s]] + [torch.from_numpy(score[d][k]).to(dev) for d in (0, 1) for k in (0, 1)]


if a.mode_ == "split":
    c = Case(2, a.side)
    for _ in range(a.calls):
        c.entries()
    torch.cuda.synchronize()
    print("%d times rsu_graph_routes of both sides and rsu_route_score in both directions at 2 x %d x %d, max_edges %d, max_nodes %d "
          "(%d and 2 launches each); info %s %s" % (a.calls, a.side, a.side, CAP, MAX_NODES, 8 + 2 * -(-MAX_NODES // 64),
                                                     c.g[0][2].cpu().numpy().tolist(), c.g[1][2].cpu().numpy().tolist()))
    sys.exit(0)

SLOW = "copy + scipy shortest_path + numpy score + copy"
FAST = "2 x rsu_graph_routes + 2 x rsu_route_score"
for S in (388, 608):
    c = Case(2, S)
    arms = [(FAST, c.entries), (SLOW, c.host_route)]
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
    print("N x H x W = 2 x %d x %d, max_edges %d, max_nodes %d, snap %d, both sides of rsu_line_segments on the pruned (min_branch %d) skeletons "
          "of two smooth road-like maps; us per call between two synchronisations, median of 20 (min .. max)" % (S, S, CAP, MAX_NODES, SNAP, BRANCH))
    for arm, u in us.items():
        print("  %-50s %11.1f us (%.1f .. %.1f), %d calls" % (arm, median(u), min(u), max(u), len(u)))
    g, score = c.host
    same = all(t.cpu().numpy().tobytes() == w.tobytes() for s in (0, 1) for t, w in zip(c.g[s], g[s])) and \
        all(c.match[d].cpu().numpy().tobytes() == score[d][0].tobytes() and c.acc[d].cpu().numpy().tolist() == score[d][1].tolist() for d in (0, 1))
    tm, hm = median(us[FAST]), median(us[SLOW])
    print("  outputs equal the host route's byte for byte: %s; %.1f us against %.1f us: x %.0f" % (same, tm, hm, hm / tm))
    info = [c.g[s][2].cpu().numpy() for s in (0, 1)]
    print("  info {nodes, stored, edges used, rows skipped} per image: prediction %s, truth %s; acc {pairs, sum q, unmatched, broken}: truth -> "
          "prediction %s, back %s; workspace %d bytes" % (info[0].tolist(), info[1].tolist(), score[0][1].tolist(), score[1][1].tolist(), c.need))
    T = -(-MAX_NODES // 64)
    for s, name in enumerate(("prediction", "truth")):
        live = [min(-(-int(k) // 64), T) for k in info[s][:, 1]]
        print("  %s: rounds with work per image %s of %d; of the %d Floyd-Warshall launches of a call (the first diagonal tile, then two per "
              "round) %s return at once for the image (the rounds past its nodes; for a graph of at most 64 nodes also round 0's two)"
              % (name, live, T, 1 + 2 * T, [2 * (T - k) + (2 if k == 1 else 0) + (1 if k == 0 else 0) for k in live]))
