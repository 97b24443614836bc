"""SHA-256 of every output buffer of every training / evaluation head entry (rsu.h rsu_head_fwd_bwd, rsu_head_fwd_bwd_w,
rsu_head_dice_sums, rsu_head_fwd_bwd_dice, rsu_head_eval; rsu_loss.h rsu_head_fwd_bwd_focal, rsu_head_eval_focal; rsu_cldice.h
rsu_head_fwd_bwd_aux) on fixed, seeded inputs: C in {16, 64}; npix not a multiple of the block's pixel count, once below and once above
the 1024-block grid limit; without weights, with class weights, with a weight map, with ignored labels; the focal entries at gamma 0 and
2, the training ones with and without the Dice sums; the aux entry with a seeded d objective / d prob and with a zero one.
For a change that must keep the bits: run it once per library (RSU_LIB_PATH), each in a fresh process, and compare the files:

    timeout -k 10 300 python tools/head_hashes.py --out a.txt
    RSU_LIB_PATH=ab_libs/librsu_parent.so timeout -k 10 300 python tools/head_hashes.py --out b.txt && cmp a.txt b.txt
"""
import argparse
import ctypes
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", required=True)
    a = ap.parse_args()
    import torch
    from road_segmentation_unet_amd._lib import EVAL_BINS, call, lib
    dev = "cuda:0"
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = []

    def digest(case, entry, **bufs):
        torch.cuda.synchronize()
        for name, t in bufs.items():
            raw = t.detach().contiguous().view(torch.int16 if t.dtype == torch.bfloat16 else t.dtype).cpu().numpy().tobytes()
            lines.append("%s %s %s %s" % (case, entry, name, hashlib.sha256(raw).hexdigest()))

    for C, npix in ((16, 40037), (64, 40037), (64, 300007)):
        gen = torch.Generator(device="cpu").manual_seed(1000 * C + npix % 1000)
        act = torch.relu(torch.randn((npix, C), generator=gen)).to(dev).to(torch.bfloat16)
        w = (torch.randn((C, 2), generator=gen) * 0.3).to(dev)
        b = (torch.randn(2, generator=gen) * 0.1).to(dev)
        labels = (torch.rand(npix, generator=gen) < 0.2).to(torch.int64)
        ignored = labels.clone()
        ignored[torch.rand(npix, generator=gen) < 0.1] = 255
        ignored[::97] = -1
        ignored[5::101] = 1 << 32   # neither 0 nor 1 only in the upper half of the 64 bits
        labels, ignored = labels.to(dev), ignored.to(dev)
        class_w = torch.tensor([0.6, 2.5], device=dev)
        pixel_w = (0.25 + torch.rand(npix, generator=gen)).to(dev)
        gprobs = {"g": (torch.randn(npix, generator=gen) * (3.0 / npix)).to(dev), "g0": torch.zeros(npix, device=dev)}
        inv = 1.0 / npix
        n_ws = max(int(lib().rsu_head_eval_ws_floats(npix, C)), int(lib().rsu_head_dice_ws_floats(npix, C)),
                   int(lib().rsu_head_w_ws_floats(npix, C)), int(lib().rsu_head_ws_floats(npix, C)))

        def fresh():
            return dict(prob=torch.zeros(npix, device=dev), dact=torch.full((npix, C), 3.0, dtype=torch.bfloat16, device=dev),
                        dw=torch.zeros((C, 2), device=dev), db=torch.zeros(2, device=dev), loss_sum=torch.zeros(1, device=dev),
                        weight_sum=torch.zeros(1, device=dev), ws=torch.zeros(n_ws, device=dev))

        o = fresh()
        call("rsu_head_fwd_bwd", p(act), p(w), p(b), p(labels), p(o["prob"]), p(o["loss_sum"]), p(o["dact"]), p(o["dw"]), p(o["db"]), p(o["ws"]),
             npix, C, inv, st)
        del o["ws"], o["weight_sum"]
        digest("C%d_n%d" % (C, npix), "fwd_bwd", **o)
        for tag, lab, cw, pw in (("plain", labels, None, None), ("class", labels, class_w, None), ("map", labels, None, pixel_w),
                                 ("class_map", labels, class_w, pixel_w), ("class_map_ignored", ignored, class_w, pixel_w)):
            case = "C%d_n%d_%s" % (C, npix, tag)
            head = (p(act), p(w), p(b), p(lab))
            o = fresh()
            call("rsu_head_fwd_bwd_w", *head, p(cw), p(pw), p(o["prob"]), p(o["loss_sum"]), p(o["weight_sum"]), p(o["dact"]), p(o["dw"]), p(o["db"]),
                 p(o["ws"]), npix, C, inv, st)
            del o["ws"]
            digest(case, "fwd_bwd_w", **o)
            o, dice_sums = fresh(), torch.full((3,), -1.0, device=dev)
            call("rsu_head_dice_sums", *head, p(pw), p(o["prob"]), p(dice_sums), p(o["ws"]), npix, C, st)
            digest(case, "dice_sums", prob=o["prob"], dice_sums=dice_sums)
            for scale in (0.0, 0.7):
                o = fresh()
                call("rsu_head_fwd_bwd_dice", *head, p(cw), p(pw), p(dice_sums), scale, 1.0, p(o["prob"]), p(o["loss_sum"]), p(o["weight_sum"]),
                     p(o["dact"]), p(o["dw"]), p(o["db"]), p(o["ws"]), npix, C, inv, st)
                del o["ws"]
                digest(case, "fwd_bwd_dice_scale%.1f" % scale, **o)
            o = fresh()
            eval_sums, eval_hist = torch.zeros(5, device=dev), torch.zeros((2, EVAL_BINS), dtype=torch.int64, device=dev)
            for _ in range(2):   # the sums and the histogram accumulate over calls
                call("rsu_head_eval", *head, p(cw), p(pw), p(o["prob"]), p(eval_sums), p(eval_hist), p(o["ws"]), npix, C, st)
            digest(case, "eval", prob=o["prob"], eval_sums=eval_sums, eval_hist=eval_hist)
            for gamma in (0.0, 2.0):
                for dtag, ds in (("", None), ("_dice", dice_sums)):
                    outs = lambda o: (p(o["prob"]), p(o["loss_sum"]), p(o["weight_sum"]), p(o["dact"]), p(o["dw"]), p(o["db"]),  # noqa: E731
                                      p(o["ws"]), npix, C, inv)
                    o = fresh()
                    call("rsu_head_fwd_bwd_focal", *head, p(cw), p(pw), gamma, p(ds), 0.7, 1.0, *outs(o), st)
                    del o["ws"]
                    digest(case, "fwd_bwd_focal_gamma%.0f%s" % (gamma, dtag), **o)
                    for gtag, gprob in gprobs.items():
                        o = fresh()
                        call("rsu_head_fwd_bwd_aux", *head, p(cw), p(pw), gamma, p(ds), 0.7, 1.0, *outs(o), p(gprob), st)
                        del o["ws"]
                        digest(case, "fwd_bwd_aux_gamma%.0f%s_%s" % (gamma, dtag, gtag), **o)
                o = fresh()
                eval_sums, eval_hist = torch.zeros(5, device=dev), torch.zeros((2, EVAL_BINS), dtype=torch.int64, device=dev)
                for _ in range(2):
                    call("rsu_head_eval_focal", *head, p(cw), p(pw), gamma, p(o["prob"]), p(eval_sums), p(eval_hist), p(o["ws"]), npix, C, st)
                digest(case, "eval_focal_gamma%.0f" % gamma, prob=o["prob"], eval_sums=eval_sums, eval_hist=eval_hist)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("%d buffers hashed with %s -> %s" % (len(lines), os.environ.get("RSU_LIB_PATH", "the product library"), a.out))


if __name__ == "__main__":
    main()
