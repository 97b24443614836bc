"""Cost of the border-distance weight map (rsu.h rsu_border_map) on the c2 geometry (N = 4, H = W = 388). Three modes; each GPU step under
its own time limit, the next only if the one before succeeded:

    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_border.py \\
      && timeout -k 10 60 python tools/bench_border.py --parse DIR >> profiles/r07/border_map.txt \\
      && timeout -k 10 300 python tools/bench_border.py --step >> profiles/r07/border_map.txt

    (no option)   issues `--warmup` + `--launches` rounds on one stream; a round is the map on each kind of labels, in this order -- "road":
                  road-like labels (a few straight roads 3 to 9 px wide per tile); "background": all-background tiles (no other class: every
                  row skips its scans); "far": one road pixel in a corner (the early-exit worst case: nearly every scan runs the full width
                  before (x - x')^2 passes its minimum); "far+mul": the same with a caller map -- and then the weighted training head
                  (rsu_head_fwd_bwd_w, C = 64) that the map feeds: the yardstick, from the same run
    --parse DIR   reads DIR/**/*kernel_trace.csv; prints the median, min and max of the map's two kernels per kind of labels and of the
                  head's kernels after the warm-up, and map / head
    --step        device time (events around `--steps` steps, `--repeats` alternating repeats) of the config-2 training step (L = 5, root
                  64, batch 4, 388 px, Momentum, no dropout) with border_weight = 10 against border_weight = 0 in the same process

The border_weight = 0 step against the parent commit is bench.py's own number from the two trees, alternating on one box."""
import argparse
import csv
import glob
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

KINDS = ["road", "background", "far", "far+mul"]


def road_labels(n, size, seed):
    """n tiles [size, size] int64: three to five straight roads, 3 to 9 px wide, at random angles"""
    import numpy as np
    rng = np.random.RandomState(seed)
    yy, xx = np.mgrid[0:size, 0:size].astype(np.float64)
    out = np.zeros((n, size, size), dtype=np.int64)
    for t in range(n):
        for _ in range(rng.randint(3, 6)):
            th, c, w = rng.uniform(0, np.pi), rng.uniform(0.1, 0.9) * size, rng.uniform(3, 9)
            out[t][np.abs(np.cos(th) * (xx - c) + np.sin(th) * (yy - c)) < w / 2] = 1
    return out


def run(args):
    import ctypes

    import numpy as np
    import torch
    from road_segmentation_unet_amd._lib import call, lib
    dev, N, P, C = "cuda:0", args.batch, args.patch, args.C
    npix = N * P * P
    far = np.zeros((N, P, P), dtype=np.int64)
    far[:, 0, 0] = 1
    road = road_labels(N, P, 3)
    labels = {"road": road, "background": np.zeros((N, P, P), np.int64), "far": far, "far+mul": far}
    labels = {k: torch.from_numpy(v).to(dev) for k, v in labels.items()}
    gen = torch.Generator(device="cpu").manual_seed(1)
    mul = (0.25 + torch.rand((N, P, P), generator=gen)).to(dev)
    out = torch.zeros((N, P, P), device=dev)
    bws = torch.zeros(int(lib().rsu_border_map_ws_bytes(N, P, P)) // 4, dtype=torch.int32, device=dev)
    act = torch.relu(torch.randn((npix, C), generator=gen)).to(dev).to(torch.bfloat16)
    w, b = (torch.randn((C, 2), generator=gen) * 0.3).to(dev), (torch.randn(2, generator=gen) * 0.1).to(dev)
    prob, dact = torch.zeros(npix, device=dev), torch.zeros((npix, C), dtype=torch.bfloat16, device=dev)
    dw, db, acc = torch.zeros((C, 2), device=dev), torch.zeros(2, device=dev), torch.zeros(2, device=dev)
    ws = torch.zeros(int(lib().rsu_head_w_ws_floats(npix, C)), device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for _ in range(args.warmup + args.launches):
        for k in KINDS:
            call("rsu_border_map", p(labels[k]), p(mul) if k == "far+mul" else None, p(out), None, p(bws), N, P, P, 10.0, 5.0, st)
        call("rsu_head_fwd_bwd_w", p(act), p(w), p(b), p(labels["road"]), None, p(out), p(prob), p(acc[0:1]), p(acc[1:2]), p(dact), p(dw), p(db),
             p(ws), npix, C, 1.0 / npix, st)
    torch.cuda.synchronize()
    print("issued %d rounds, N %d H = W %d; road fraction of the road-like labels %.3f" % (args.warmup + args.launches, N, P, float(road.mean())))


def parse(args):
    rows = []
    for f in glob.glob(os.path.join(args.parse, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    t, n = {}, {"cols": 0, "rows": 0}
    for s, e, name in rows:
        us = (e - s) / 1e3
        for part in ("cols", "rows"):
            if "k_border_" + part in name:
                t.setdefault((KINDS[n[part] % len(KINDS)], part), []).append(us)
                n[part] += 1
        if "k_head_final" in name:
            t.setdefault(("head", "final"), []).append(us)
        elif "k_head" in name:
            t.setdefault(("head", "main"), []).append(us)
    med = {}
    print("border map kernels, N %d x %d x %d, after %d warm-up rounds (rocprofv3 kernel trace; us)" % (args.batch, args.patch, args.patch, args.warmup))
    for key in [(k, part) for k in KINDS for part in ("cols", "rows")] + [("head", "main"), ("head", "final")]:
        v = t.get(key, [])[args.warmup:]
        if len(v) < 20:
            raise SystemExit("%s: %d launches after warm-up, need >= 20" % (key, len(v)))
        med[key] = statistics.median(v)
        print("%-11s %-6s n %3d  median %8.2f  min %8.2f  max %8.2f" % (key[0], key[1], len(v), med[key], min(v), max(v)))
    head = med["head", "main"] + med["head", "final"]
    for k in KINDS:
        m = med[k, "cols"] + med[k, "rows"]
        print("map on %-11s %7.2f us = %.3f x the weighted head it feeds (k_head + final, %.2f us)" % (k, m, m / head, head))
    return 0


def step(args):
    import torch
    from road_segmentation_unet_amd.unet import UNet
    L, root, B, P = 5, 64, args.batch, args.patch
    nets = {}
    for w0 in (0.0, 10.0):
        m = nets[w0] = UNet(L, root, False, B, P, seed=7, training=True, border_weight=w0)
        gen = torch.Generator(device="cpu").manual_seed(2)
        m.x.copy_(torch.rand(tuple(m.x.shape), generator=gen))
        m.labels.copy_(torch.from_numpy(road_labels(B, P, 3)))
        m.ensure_tuned()
    inv = 1.0 / (B * P * P)

    def steps(m, k):
        for _ in range(k):
            m.forward_device()
            m.backward_device(inv)
            m.apply_momentum(0.0, 0.9)
    ms = {0.0: [], 10.0: []}
    for w0 in nets:
        steps(nets[w0], args.warmup)
    for _ in range(args.repeats):
        for w0, m in nets.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            steps(m, args.steps)
            e1.record()
            torch.cuda.synchronize()
            ms[w0].append(e0.elapsed_time(e1) / args.steps)
    print("config-2 training step (L 5, root 64, batch %d, %d px, Momentum, no dropout), %d alternating repeats of %d steps, device ms per step"
          % (B, P, args.repeats, args.steps))
    for w0 in ms:
        print("border_weight %4.1f: median %.4f  min %.4f  max %.4f   %s" % (w0, statistics.median(ms[w0]), min(ms[w0]), max(ms[w0]),
                                                                            " ".join("%.4f" % v for v in ms[w0])))
    a, b = statistics.median(ms[0.0]), statistics.median(ms[10.0])
    print("border_weight 10 / 0: %.4f (+%.1f us per step; weight sum of the last step %.0f over %d pixels)"
          % (b / a, (b - a) * 1e3, float(nets[10.0].weight_sum), B * P * P))
    return 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parse", metavar="DIR", default=None)
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--patch", type=int, default=388)
    ap.add_argument("--C", type=int, default=64)
    a = ap.parse_args()
    sys.exit(parse(a) if a.parse else step(a) if a.step else run(a))
