"""Time of the evaluation head (rsu.h rsu_head_eval) next to the two calls it shares its reads with, rsu_head_dice_sums (forward only,
three sums) and rsu_head_fwd_bwd_w (the weighted training head, which also writes dact), on the c2 geometry (npix = 4 * 388 * 388,
C = 64), for two input distributions: probabilities uniform in [0, 1] (every histogram bin in use) and saturated ones (weights x 40:
nearly every pixel in bin 0 or bin 255, where same-address contention would show). Run it under its own time limit:

    timeout -k 10 300 python tools/bench_head_eval.py --out profiles/r07/head_eval.json

Per distribution: `--warmup` launches of each call, then `--rounds` rounds; a round times `--launches` back-to-back launches of each
call between two events (the call's main and final kernels together), the three calls in turn, so that clock and box drift hit all
three alike. The figure of a call is the median over the rounds of (elapsed / launches). Exit status 1 if rsu_head_eval is slower than
rsu_head_fwd_bwd_w for either distribution (it reads the same bytes and does not write dact); its ratio to rsu_head_dice_sums and the
saturated / uniform ratio are reported, not gated."""
import argparse
import ctypes
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def inputs(kind, npix, C, dev):
    import torch
    gen = torch.Generator(device="cpu").manual_seed(1)
    act = torch.relu(torch.randn((npix, C), generator=gen))
    if kind == "uniform":
        # logit difference t = logit(u) carried by channels 0 / 1 (ReLU activations: the positive and the negative part), no other weight
        u = torch.rand(npix, generator=gen).clamp_(1e-4, 1.0 - 1e-4)
        t = torch.log(u) - torch.log1p(-u)
        act[:, 0], act[:, 1] = torch.relu(t), torch.relu(-t)
        w = torch.zeros((C, 2))
        w[0, 0], w[0, 1], w[1, 0], w[1, 1] = -0.5, 0.5, 0.5, -0.5
        b = torch.zeros(2)
    else:
        w = torch.randn((C, 2), generator=gen) * 0.3 * 40.0
        b = torch.randn(2, generator=gen) * 0.1
    labels = (torch.rand(npix, generator=gen) < 0.2).to(torch.int64)
    pixel_w = 0.25 + torch.rand(npix, generator=gen)
    return act.to(dev).to(torch.bfloat16), w.to(dev), b.to(dev), labels.to(dev), pixel_w.to(dev)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", default=None, help="write the result as JSON here")
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--patch", type=int, default=388)
    ap.add_argument("--C", type=int, default=64)
    a = ap.parse_args()
    import torch
    from road_segmentation_unet_amd._lib import EVAL_BINS, call, lib
    dev, C, npix = "cuda:0", a.C, a.batch * a.patch * a.patch
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    class_w = torch.tensor([0.6, 2.5], device=dev)
    prob, dact = torch.zeros(npix, device=dev), torch.zeros((npix, C), dtype=torch.bfloat16, device=dev)
    dw, db, acc, dsums = torch.zeros((C, 2), device=dev), torch.zeros(2, device=dev), torch.zeros(2, device=dev), torch.zeros(3, device=dev)
    esums, hist = torch.zeros(5, device=dev), torch.zeros((2, EVAL_BINS), dtype=torch.int64, device=dev)
    n_ws = max(int(lib().rsu_head_eval_ws_floats(npix, C)), int(lib().rsu_head_dice_ws_floats(npix, C)))
    ws = torch.zeros(n_ws, device=dev)
    result = {"npix": npix, "C": C, "launches": a.launches, "rounds": a.rounds, "warmup": a.warmup, "device": torch.cuda.get_device_name(0)}
    ok = True
    for kind in ("uniform", "saturated"):
        act, w, b, labels, pixel_w = inputs(kind, npix, C, dev)
        head = (p(act), p(w), p(b), p(labels))
        calls = {
            "rsu_head_eval": lambda: call("rsu_head_eval", *head, p(class_w), p(pixel_w), p(prob), p(esums), p(hist), p(ws), npix, C, st),
            "rsu_head_dice_sums": lambda: call("rsu_head_dice_sums", *head, p(pixel_w), p(prob), p(dsums), p(ws), npix, C, st),
            "rsu_head_fwd_bwd_w": lambda: call("rsu_head_fwd_bwd_w", *head, p(class_w), p(pixel_w), p(prob), p(acc[0:1]), p(acc[1:2]), p(dact),
                                               p(dw), p(db), p(ws), npix, C, 1.0 / npix, st),
        }
        hist.zero_()
        calls["rsu_head_eval"]()
        torch.cuda.synchronize()
        h = hist.sum(0).cpu().numpy().astype(float)
        ends = float(h[0] + h[-1]) / float(h.sum())
        for f in calls.values():
            for _ in range(a.warmup):
                f()
        torch.cuda.synchronize()
        us = {k: [] for k in calls}
        for _ in range(a.rounds):
            for k, f in calls.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.launches):
                    f()
                e1.record()
                e1.synchronize()
                us[k].append(1e3 * e0.elapsed_time(e1) / a.launches)
        med = {k: statistics.median(v) for k, v in us.items()}
        r = {"us_per_call": med, "us_per_call_rounds": us, "fraction_in_bins_0_and_255": ends, "bins_in_use": int((h > 0).sum()),
             "eval_over_fwd_bwd_w": med["rsu_head_eval"] / med["rsu_head_fwd_bwd_w"],
             "eval_over_dice_sums": med["rsu_head_eval"] / med["rsu_head_dice_sums"]}
        result[kind] = r
        print("%-9s (%.1f %% of the pixels in bins 0 and 255, %d bins in use): eval %.2f us, dice_sums %.2f us, fwd_bwd_w %.2f us; "
              "eval / fwd_bwd_w %.3f, eval / dice_sums %.3f" % (kind, 100 * ends, r["bins_in_use"], med["rsu_head_eval"], med["rsu_head_dice_sums"],
                                                              med["rsu_head_fwd_bwd_w"], r["eval_over_fwd_bwd_w"], r["eval_over_dice_sums"]))
        ok = ok and med["rsu_head_eval"] <= med["rsu_head_fwd_bwd_w"]
    result["saturated_over_uniform_eval"] = result["saturated"]["us_per_call"]["rsu_head_eval"] / result["uniform"]["us_per_call"]["rsu_head_eval"]
    result["eval_not_slower_than_fwd_bwd_w"] = ok
    print("saturated / uniform (rsu_head_eval): %.3f; not slower than rsu_head_fwd_bwd_w: %s" % (result["saturated_over_uniform_eval"], ok))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
