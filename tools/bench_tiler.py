#!/usr/bin/env python3
"""The tiler kernels alone: rsu_extract_tiles / rsu_overlap_add against rsu_extract_tiles_rect / rsu_overlap_add_rect on one geometry
(default: c5's -- six 604 x 604 image variants, P = 388, S = 764, stride 12, 2166 tiles; extract of one batch of 8 tiles, overlap-add of
all tiles in one call, as predict()'s shared-window path issues it). Event-timed, arms alternated over --rounds, median of --reps each.
usage: python tools/bench_tiler.py [--size 604 --P 388 --S 764 --stride 12 --images 6 --batch 8]"""
import argparse, ctypes, os, statistics, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from road_segmentation_unet_amd._lib import call
ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=604); ap.add_argument("--P", type=int, default=388); ap.add_argument("--S", type=int, default=764)
ap.add_argument("--stride", type=int, default=12); ap.add_argument("--images", type=int, default=6); ap.add_argument("--batch", type=int, default=8)
ap.add_argument("--rounds", type=int, default=5); ap.add_argument("--reps", type=int, default=20)
a = ap.parse_args()
H, P, S, s, n = a.size, a.P, a.S, a.stride, a.images
assert (H - P) % s == 0, "the square entries need a stride that covers the image"
pps = (H - P) // s + 1
nt = n * pps * pps
dev = "cuda:0"
imgs = torch.rand((n, H, H, 3), device=dev)
x = torch.empty((a.batch, S, S, 3), device=dev)
prob = torch.rand((nt, P, P), device=dev)
acc, hits = torch.zeros((n, H, H), device=dev), torch.zeros((n, H, H), device=dev)
ptr = lambda t: ctypes.c_void_p(t.data_ptr())
st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
t0 = nt // 2
arms = {
    "extract": lambda: call("rsu_extract_tiles", ptr(imgs), ptr(x), n, H, S, P, s, t0, a.batch, st),
    "extract_rect": lambda: call("rsu_extract_tiles_rect", ptr(imgs), ptr(x), n, H, H, S, P, s, t0, a.batch, st),
    "overlap_add": lambda: call("rsu_overlap_add", ptr(prob), ptr(acc), ptr(hits), n, H, P, s, 0, nt, st),
    "overlap_add_rect": lambda: call("rsu_overlap_add_rect", ptr(prob), ptr(acc), ptr(hits), n, H, H, P, s, 0, nt, st),
}


def timed(fn):
    out = []
    for _ in range(a.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) * 1e3)
    return statistics.median(out)


for fn in arms.values():
    fn()
torch.cuda.synchronize()
res = {k: [] for k in arms}
for _ in range(a.rounds):
    for k, fn in arms.items():
        res[k].append(timed(fn))
print({"geometry": {"images": n, "size": H, "P": P, "S": S, "stride": s, "tiles": nt, "extract_batch": a.batch},
       "median_us_per_round": {k: [round(v, 1) for v in vs] for k, vs in res.items()}})
