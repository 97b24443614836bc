"""Kernel time of every head variant (rsu.h rsu_head_fwd_bwd, rsu_head_fwd_bwd_w, rsu_head_dice_sums + rsu_head_fwd_bwd_dice,
rsu_head_eval) on the c2 geometry (npix = 4 * 388 * 388, C = 64). Two modes, each step under its own time limit, the second only if
the first succeeded:

    timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_head.py \\
      && timeout -k 10 60 python tools/bench_head.py --parse DIR

    (no --parse)  issues `--warmup` + `--launches` rounds on one stream; a round is, in this order: U the unweighted training head,
                  Wc the weighted one with class weights only, Wm with class weights and a weight map, A + B the two passes of the
                  soft-Dice head (weights + map), E the evaluation head (weights + map), Es the same on saturated probabilities (head
                  weights x 40: nearly every pixel in histogram bin 0 or 255, where same-address contention would show)
    --parse DIR   reads DIR/**/*kernel_trace.csv; prints the median, min, max and spread of each main and final kernel after the warm-up
                  and the derived ratios next to the byte ratios they are expected to follow. Exit status 1 if the evaluation head is
                  slower than the weighted training head (it reads the same bytes and does not write dact).

The name table knows every name these kernels have had (kernels of their own; k_head_loss<DICE> / k_head_sums<EVAL>; now
k_head_train<FOCAL, DICE, AUX> / k_head_sums<EVAL, FOCAL>), so a trace of either library (RSU_LIB_PATH) parses."""
import argparse
import csv
import glob
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

# kernel name (demangled or mangled; first match wins) -> kind. A final kernel belongs to the main kernel issued just before it.
NAMES = [("k_head_final", "final"), ("k_head_eval_final", "final"),
         ("k_head_dice_sums", "A"), ("k_head_sums<false", "A"), ("k_head_sumsILb0", "A"),
         ("k_head_dice", "B"), ("k_head_loss<true>", "B"), ("k_head_lossILb1", "B"), ("k_head_train<false, true, false>", "B"),
         ("k_head_trainILb0ELb1ELb0", "B"),
         ("k_head_w", "W"), ("k_head_loss<false>", "W"), ("k_head_lossILb0", "W"), ("k_head_train<false, false, false>", "W"),
         ("k_head_trainILb0ELb0ELb0", "W"),
         ("k_head_eval", "E"), ("k_head_sums<true", "E"), ("k_head_sumsILb1", "E"),
         ("k_head<true>", "U"), ("k_headILb1", "U")]
ROUND = {"U": ["U"], "W": ["Wc", "Wm"], "A": ["A"], "B": ["B"], "E": ["E", "Es"]}   # the dispatches of one kind within a round, in issue order
WHAT = {"U": "unweighted", "Wc": "weighted, class weights", "Wm": "weighted, class weights + map", "A": "Dice pass A (sums)",
        "B": "Dice pass B", "E": "evaluation", "Es": "evaluation, saturated"}


def run(args):
    import ctypes

    import torch
    from road_segmentation_unet_amd._lib import EVAL_BINS, call, lib
    dev, C, npix = "cuda:0", args.C, args.batch * args.patch * args.patch
    gen = torch.Generator(device="cpu").manual_seed(1)
    act = torch.relu(torch.randn((npix, C), generator=gen)).to(dev).to(torch.bfloat16)
    w = (torch.randn((C, 2), generator=gen) * 0.3).to(dev)
    b = (torch.randn(2, generator=gen) * 0.1).to(dev)
    labels = (torch.rand(npix, generator=gen) < 0.2).to(torch.int64).to(dev)
    class_w = torch.tensor([0.6, 2.5], device=dev)
    pixel_w = (0.25 + torch.rand(npix, generator=gen)).to(dev)
    w_sat = w * 40.0
    prob, dact = torch.zeros(npix, device=dev), torch.zeros((npix, C), dtype=torch.bfloat16, device=dev)
    dw, db, acc, sums = torch.zeros((C, 2), device=dev), torch.zeros(2, device=dev), torch.zeros(2, device=dev), torch.zeros(3, device=dev)
    esums, hist = torch.zeros(5, device=dev), torch.zeros((2, EVAL_BINS), dtype=torch.int64, device=dev)
    ws = torch.zeros(max(int(lib().rsu_head_eval_ws_floats(npix, C)), int(lib().rsu_head_dice_ws_floats(npix, C))), device=dev)
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    inv = 1.0 / npix
    head = (p(act), p(w), p(b), p(labels))
    grads = (p(dact), p(dw), p(db), p(ws), npix, C, inv, st)
    for _ in range(args.warmup + args.launches):
        call("rsu_head_fwd_bwd", *head, p(prob), p(acc[0:1]), *grads)
        for pw in (None, pixel_w):
            call("rsu_head_fwd_bwd_w", *head, p(class_w), p(pw), p(prob), p(acc[0:1]), p(acc[1:2]), *grads)
        call("rsu_head_dice_sums", *head, p(pixel_w), p(prob), p(sums), p(ws), npix, C, st)
        call("rsu_head_fwd_bwd_dice", *head, p(class_w), p(pixel_w), p(sums), 0.7, 1.0, p(prob), p(acc[0:1]), p(acc[1:2]), *grads)
        for ww in (w, w_sat):
            call("rsu_head_eval", p(act), p(ww), p(b), p(labels), p(class_w), p(pixel_w), p(prob), p(esums), p(hist), p(ws), npix, C, st)
    torch.cuda.synchronize()
    print("issued %d rounds of head launches, npix %d C %d, library %s; dice_sums %s"
          % (args.warmup + args.launches, npix, C, os.environ.get("RSU_LIB_PATH", "(product)"), sums.cpu().tolist()))


def parse(args):
    rows = []
    for f in glob.glob(os.path.join(args.parse, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            for r in csv.DictReader(fh):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]))
    rows.sort()
    t, seen, count, last = {}, {}, {k: 0 for k in ROUND}, None
    for s, e, name in rows:
        kind = next((k for pat, k in NAMES if pat in name), None)
        if kind is None or (kind == "final" and last is None):
            continue
        if kind == "final":
            key = "F" + last
        else:
            key = last = ROUND[kind][count[kind] % len(ROUND[kind])]
            count[kind] += 1
        t.setdefault(key, []).append((e - s) / 1e3)
        seen[key] = name.split("(")[0].replace("void ", "")
    med = {}
    for k in WHAT:
        for key in (k, "F" + k):
            v = t.get(key, [])[args.warmup:]
            if len(v) < 20:
                raise SystemExit("%s: %d launches after warm-up, need >= 20" % (key, len(v)))
            med[key] = statistics.median(v)
            print("%-3s %-30s %-24s n %3d  median %8.2f us  min %8.2f  max %8.2f  spread (max-min)/median %.1f %%"
                  % (key, WHAT[k] + (", final" if key != k else ""), seen[key], len(v), med[key], min(v), max(v),
                     100.0 * (max(v) - min(v)) / med[key]))
    C = args.C
    base = 4.0 * C + 8 + 4      # per pixel: bf16 activations in + bf16 dact out, the int64 label, the probability
    fwd = 2.0 * C + 8 + 4 + 4   # forward only, with the weight map: no dact
    full = lambda k: med[k] + med["F" + k]  # noqa: E731
    print("Wc / U %.4f (bytes: 1.0000)   Wm / U %.4f (bytes: %.4f = +4 B on %d B per pixel)" % (med["Wc"] / med["U"], med["Wm"] / med["U"],
                                                                                            (base + 4) / base, int(base)))
    print("weighted head %.2f us; Dice pair %.2f us = %.4f x (bytes: %.4f = %d + %d B on %d B per pixel); pass B / Wm %.4f"
          % (full("Wm"), full("A") + full("B"), (full("A") + full("B")) / full("Wm"), (base + 4 + fwd) / (base + 4), int(fwd), int(base + 4),
             int(base + 4), med["B"] / med["Wm"]))
    ok = full("E") <= full("Wm") and full("Es") <= full("Wm")
    print("evaluation head %.2f us (saturated %.2f us, x %.4f); / weighted head %.4f; / Dice pass A %.4f; not slower than the weighted head: %s"
          % (full("E"), full("Es"), full("Es") / full("E"), full("E") / full("Wm"), full("E") / full("A"), ok))
    return 0 if ok else 1


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parse", metavar="DIR", default=None)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--patch", type=int, default=388)
    ap.add_argument("--C", type=int, default=64)
    a = ap.parse_args()
    sys.exit(parse(a) if a.parse else run(a))
