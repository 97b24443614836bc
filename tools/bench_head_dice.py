"""Kernel time of the head's training launches with and without the soft-Dice term (rsu.h rsu_head_fwd_bwd, rsu_head_fwd_bwd_w,
rsu_head_dice_sums + rsu_head_fwd_bwd_dice), on the c2 geometry (npix = 4 * 388 * 388, C = 64). Two modes, each step under its own time
limit, the second only if the first succeeded:

    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_head_dice.py \\
      && timeout -k 10 60 python tools/bench_head_dice.py --parse DIR

    (no --parse)  issues, round robin on one stream: A k_head<true>, B k_head_w (class weights + weight map), C the Dice pair
                  k_head_dice_sums, k_head_dice (class weights + weight map) with its two final kernels; `--warmup` + `--launches` of each
    --parse DIR   reads DIR/**/*kernel_trace.csv; prints the median, min and max of each kernel after the warm-up, the Dice pair's sum
                  against k_head_w, and the byte ratio it is expected to follow
"""
import argparse
import csv
import glob
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# (first match wins: the final kernels' names contain the main kernels' names)
KERNELS = [("k_head_final_dice_sums", "FA"), ("k_head_final_dice", "FB"), ("k_head_final_w", "FW"), ("k_head_final", "FU"),
           ("k_head_dice_sums", "A"), ("k_head_dice", "B"), ("k_head_w", "W"), ("k_head<true>", "U"), ("k_headILb1", "U")]
WHAT = {"U": "k_head<true> (unweighted)", "W": "k_head_w (class weights + map)", "A": "k_head_dice_sums (pass A)", "B": "k_head_dice (pass B)",
        "FU": "k_head_final", "FW": "k_head_final_w", "FA": "k_head_final_dice_sums", "FB": "k_head_final_dice"}


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
    dw, db, acc, sums = torch.zeros((C, 2), device=dev), torch.zeros(2, device=dev), torch.zeros(2, device=dev), torch.zeros(3, device=dev)
    ws = torch.zeros(int(lib().rsu_head_dice_ws_floats(npix, C)), device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    inv = 1.0 / npix
    head = (p(act), p(w), p(b), p(labels))
    for _ in range(args.warmup + args.launches):
        call("rsu_head_fwd_bwd", *head, p(prob), p(acc[0:1]), p(dact), p(dw), p(db), p(ws), npix, C, inv, st)
        call("rsu_head_fwd_bwd_w", *head, p(class_w), p(pixel_w), p(prob), p(acc[0:1]), p(acc[1:2]), p(dact), p(dw), p(db), p(ws), npix, C, inv, st)
        call("rsu_head_dice_sums", *head, p(pixel_w), p(prob), p(sums), p(ws), npix, C, st)
        call("rsu_head_fwd_bwd_dice", *head, p(class_w), p(pixel_w), p(sums), 0.7, 1.0, p(prob), p(acc[0:1]), p(acc[1:2]), p(dact), p(dw), p(db),
             p(ws), npix, C, inv, st)
    torch.cuda.synchronize()
    print("issued %d x (unweighted, weighted, Dice pair) head launches, npix %d C %d; dice_sums %s" % (args.warmup + args.launches, npix, C,
                                                                                                      sums.cpu().tolist()))


def parse(args):
    rows = []
    for f in glob.glob(os.path.join(args.parse, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    t = {k: [] for k in WHAT}
    for s, e, name in rows:
        for pat, key in KERNELS:
            if pat in name:
                t[key].append((e - s) / 1e3)
                break
    med = {}
    for k in ("U", "FU", "W", "FW", "A", "FA", "B", "FB"):
        v = t[k][args.warmup:]
        if len(v) < 20:
            raise SystemExit("%s: %d launches after warm-up, need >= 20" % (WHAT[k], len(v)))
        med[k] = statistics.median(v)
        print("%-34s n %3d  median %8.2f us  min %8.2f  max %8.2f  spread (max-min)/median %.1f %%"
              % (WHAT[k], len(v), med[k], min(v), max(v), 100.0 * (max(v) - min(v)) / med[k]))
    C = args.C
    one = 4.0 * C + 8 + 4 + 4      # per pixel: bf16 activations in + bf16 dact out, the int64 label, the weight, the probability
    sums = 2.0 * C + 8 + 4 + 4     # pass A: no dact
    pair, wtd = med["A"] + med["FA"] + med["B"] + med["FB"], med["W"] + med["FW"]
    print("weighted head %.2f us; Dice pair %.2f us = %.4f x (bytes: %.4f = %d + %d B on %d B per pixel); pass B / k_head_w %.4f; "
          "k_head_w / k_head<true> %.4f" % (wtd, pair, pair / wtd, (one + sums) / one, int(sums), int(one), int(one), med["B"] / med["W"],
                                           med["W"] / med["U"]))


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
