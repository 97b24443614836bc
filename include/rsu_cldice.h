/*
 * rsu_cldice.h -- the fourth public header of librsu_hip.so: the clDice (centre-line Dice) loss term with fused soft-skeleton kernels.
 *
 * Same library, same conventions and memory contract as rsu.h (plain C, device pointers + sizes, `stream` a hipStream_t passed as void*,
 * asynchronous on that stream, 0 on success and a negative RSU_E* code otherwise). tests/test_gpu_cldice_fenced.py holds every launching
 * entry of this header to the memory contract; road_segmentation_unet_amd/_lib.py binds it through its table SIGNATURES_CLDICE.
 */
#ifndef RSU_CLDICE_H_
#define RSU_CLDICE_H_

#include "rsu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- clDice (new; the reference has none): Shit et al., CVPR 2021, soft_skel / soft_cldice -------- */
/* The heads' losses are per-pixel or area-overlap objectives; this term sees connectivity: how much of the predicted centre line lies
 * inside the true mask and how much of the true centre line inside the predicted mask, both centre lines soft skeletons. All float32.
 * p = prob [B][H][W] (what the heads write), labels int64 [B][H][W]; y = 1 where the label is 1, else 0; m = 1 where the label is 0 or 1
 * (all 64 bits tested), else 0, applied by selection; k = iters; s = smooth.
 *   erode(x)[r,c]  = min over the cross {(r-1,c), (r,c-1), (r,c), (r,c+1), (r+1,c)};  dilate(x)[r,c] = max over the 3 x 3 box, row-major
 *   (positions outside the image do not exist; no window crosses into another image)
 *   E_0 = x, E_j = erode(E_{j-1});  d_j = relu(E_j - dilate(erode(E_j))), j = 0..k
 *   S_0 = d_0, S_j = S_{j-1} + relu(d_j - S_{j-1} * d_j);  skel(x) = S_k            (one rounding per operation, nothing fused)
 *   A = sum m skel(p) y,  Bp = sum m skel(p),  Cc = sum m skel(y) p,  Dy = sum m skel(y)      (over the call's B images)
 *   Tp = (A + s) / (Bp + s),  Ts = (Cc + s) / (Dy + s),  clD = 2 Tp Ts / (Tp + Ts);   the term is scale * (1 - clD)
 * Gradient wrt p: the direct part -scale dclD/dTs m skel(y) / (Dy + s), plus G = -scale dclD/dTp m (y (Bp + s) - (A + s)) / (Bp + s)^2
 * chained back through the S recursion, the openings and the erosions; dclD/dTp = 2 Ts^2 / (Tp + Ts)^2, dclD/dTs = 2 Tp^2 / (Tp + Ts)^2.
 * The sub-gradient is pinned: among equal candidates of a window the FIRST in the window's row-major order wins, by strict comparisons
 * (cross: up, left, centre, right, down), and relu'(0) = 0. Ignored pixels (m = 0) are constants of the skeleton: their p takes part in
 * the pooling, they add nothing to the sums and their gprob is 0. hostio.soft_skeleton / hostio.cldice_gradient restate all of it.
 *
 * rsu_cldice_fwd: skel_p, skel_y [B][H][W] are overwritten; sums[0..3] += {A, Bp, Cc, Dy} (the caller zeroes). Two launches whatever
 *   iters: the tiled skeleton kernel and a final kernel that adds the tiles' partial sums in a fixed order. ws: rsu_cldice_ws_floats floats.
 *   ws need not be cleared and the forward reads nothing it did not write itself. It WRITES, for the backward: the erosion levels
 *   E_1 .. E_{iters+1} and the skeleton states S_0 .. S_{iters-1} of the prob map, [2 iters + 1][B H W] floats, and behind them the
 *   tiles' partial sums, which only its own final kernel reads.
 * rsu_cldice_bwd: gprob [B][H][W] is overwritten with d (scale (1 - clD)) / d p, with the sums READ from `sums` as they stand (what the
 *   forward left, or what a host made of it: nothing is recomputed). One launch whatever iters; no atomics, a fixed order of every sum.
 *   It reads what rsu_cldice_fwd left in ws for the same prob, labels and iters -- those [2 iters + 1] maps, nothing else -- and writes
 *   nothing to it: the caller leaves ws untouched between the two. This is the one workspace that carries data from one entry to another;
 *   behind the backward, and in front of the next forward, it holds nothing.
 *   skel_p is part of the signature for symmetry and is not read.
 * No host synchronisation anywhere. Errors, returned before anything is launched or written: RSU_EINVAL for a NULL pointer, B, H, W < 1,
 * B * H * W >= 2^31, iters outside [0, RSU_CLDICE_MAX_ITERS], a smooth that is not finite and > 0, a scale that is not finite and >= 0. */
#define RSU_CLDICE_MAX_ITERS 16
size_t rsu_cldice_ws_floats(int B, int H, int W, int iters);   /* 0 for refused arguments */
/* align (rsu_cldice_fwd): prob 4, labels 8, skel_p 4, skel_y 4, sums 4, ws 4. */
int rsu_cldice_fwd(const float* prob, const int64_t* labels, int iters, float* skel_p, float* skel_y, float* sums, float* ws, int B, int H,
                   int W, rsu_stream_t stream);
/* align (rsu_cldice_bwd): prob 4, labels 8, skel_p 4, skel_y 4, sums 4, gprob 4, ws 4. */
int rsu_cldice_bwd(const float* prob, const int64_t* labels, const float* skel_p, const float* skel_y, const float* sums, int iters,
                   float scale, float smooth, float* gprob, float* ws, int B, int H, int W, rsu_stream_t stream);

/* rsu_head_fwd_bwd_aux: rsu_head_fwd_bwd_focal (rsu_loss.h) with a given gradient of a further term wrt prob: for every counted pixel
 * gprob[p] * p0 p1 is added to dlogit 1 and taken from dlogit 0 (p1 = softmax(z)[1]) in front of dact, dw and db. An ignored pixel's
 * gprob is not looked at (its dact row is +0). loss_sum and weight_sum keep their meaning: the cross-entropy part only. gamma == 0 is
 * allowed and gives the cross-entropy lines of rsu_head_fwd_bwd_w / rsu_head_fwd_bwd_dice; every other argument, the workspace
 * (rsu_head_dice_ws_floats; it need not be cleared and holds nothing between calls) and every other error are rsu_head_fwd_bwd_focal's; a NULL gprob is RSU_EINVAL. With gprob all zero every
 * output equals that entry's as numbers. */
/* align (rsu_head_fwd_bwd_aux): act 16, w 4, b 4, labels 8, class_w 4, pixel_w 4, dice_sums 4, prob 4, loss_sum 4, weight_sum 4, dact 16, dw 4,
 * db 4, ws 4, gprob 4. */
int rsu_head_fwd_bwd_aux(const void* act, const float* w, const float* b, const int64_t* labels, const float* class_w /* may be NULL */,
                         const float* pixel_w /* may be NULL */, float gamma, const float* dice_sums /* may be NULL */, float dice_scale,
                         float smooth, float* prob, float* loss_sum, float* weight_sum /* may be NULL */, void* dact, float* dw, float* db,
                         float* ws, long npix, int C, float inv_count, const float* gprob, rsu_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RSU_CLDICE_H_ */
