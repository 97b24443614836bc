"""Kernel time of the head's training launch, unweighted against weighted (rsu.h rsu_head_fwd_bwd / rsu_head_fwd_bwd_w), on the c2
geometry (npix = 4 * 388 * 388, C = 64). Two modes:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_head_weighted.py
        issues, round robin on one stream: A k_head<true>, B k_head_w with class weights only, C k_head_w with class weights and a
        weight map; `--warmup` + `--launches` of each
    python tools/bench_head_weighted.py --parse DIR
        reads DIR/**/*kernel_trace.csv: the k_head_w dispatches alternate B, C in issue order; prints the median, min and max of each
        variant after the warm-up, the ratios B / A and C / A, and the byte ratio they are expected to follow
"""
import argparse
import csv
import glob
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(args):
    import ctypes

    import torch
    from road_segmentation_unet_amd._lib import call, lib
    dev, C, npix = "cuda:0", args.C, args.batch * args.patch * args.patch
    gen = torch.Generator(device="cpu").manual_seed(1)
    act = torch.relu(torch.randn((npix, C), generator=gen)).to(dev).to(torch.bfloat16)
    w = (torch.randn((C, 2), generator=gen) * 0.3).to(dev)
    b = (torch.randn(2, generator=gen) * 0.1).to(dev)
    labels = (torch.rand(npix, generator=gen) < 0.2).to(torch.int64).to(dev)
    class_w = torch.tensor([0.6, 2.5], device=dev)
    pixel_w = (0.25 + torch.rand(npix, generator=gen)).to(dev)
    prob, dact = torch.zeros(npix, device=dev), torch.zeros((npix, C), dtype=torch.bfloat16, device=dev)
    dw, db, acc = torch.zeros((C, 2), device=dev), torch.zeros(2, device=dev), torch.zeros(2, device=dev)
    ws = torch.zeros(int(lib().rsu_head_w_ws_floats(npix, C)), device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    inv = 1.0 / npix
    for _ in range(args.warmup + args.launches):
        call("rsu_head_fwd_bwd", p(act), p(w), p(b), p(labels), p(prob), p(acc[0:1]), p(dact), p(dw), p(db), p(ws), npix, C, inv, st)
        for pw in (None, pixel_w):
            call("rsu_head_fwd_bwd_w", p(act), p(w), p(b), p(labels), p(class_w), p(pw), p(prob), p(acc[0:1]), p(acc[1:2]), p(dact), p(dw), p(db),
                 p(ws), npix, C, inv, st)
    torch.cuda.synchronize()
    print("issued %d x 3 head launches, npix %d C %d" % (args.warmup + args.launches, npix, C))


def parse(args):
    rows = []
    for f in glob.glob(os.path.join(args.parse, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    t = {"A": [], "B": [], "C": []}
    nw = 0
    for s, e, name in rows:
        if "k_head_final" in name:
            continue
        if "k_head_w" in name:
            t["BC"[nw & 1]].append((e - s) / 1e3)
            nw += 1
        elif "k_head<true>" in name or "k_headILb1" in name:
            t["A"].append((e - s) / 1e3)
    what = {"A": "k_head<true> (unweighted)", "B": "k_head_w, class weights only", "C": "k_head_w, class weights + weight map"}
    med = {}
    for k in "ABC":
        v = t[k][args.warmup:]
        if len(v) < 20:
            raise SystemExit("variant %s: %d launches after warm-up, need >= 20" % (k, len(v)))
        med[k] = statistics.median(v)
        print("%-40s n %3d  median %8.2f us  min %8.2f  max %8.2f  spread (max-min)/median %.1f %%"
              % (what[k], len(v), med[k], min(v), max(v), 100.0 * (max(v) - min(v)) / med[k]))
    C = args.C
    base = 4.0 * C + 8 + 4      # per pixel: bf16 activations in + bf16 dact out, the int64 label, the probability
    print("ratio B / A %.4f (bytes: %.4f)   ratio C / A %.4f (bytes: %.4f = +4 B on %d B per pixel)"
          % (med["B"] / med["A"], 1.0, med["C"] / med["A"], (base + 4) / base, int(base)))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parse", metavar="DIR", default=None)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--patch", type=int, default=388)
    ap.add_argument("--C", type=int, default=64)
    a = ap.parse_args()
    parse(a) if a.parse else run(a)
