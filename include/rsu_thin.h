/*
 * rsu_thin.h -- the eighth public header of librsu_hip.so: the centre-line of a predicted mask and of a truth mask, on the device, by
 * Guo & Hall's two-sub-iteration parallel thinning, and the four counts from which the host reads the clDice METRIC on hard skeletons.
 * Its two outputs are written in the formats rsu_distance_hist, rsu_components_pair_count and the mask pipeline read, so the distance
 * histogram of two skeletons gives the completeness, correctness and quality of the road-extraction literature at every slack at once.
 *
 * Same library, same conventions and memory contract as rsu.h and rsu_distance.h (plain C, device pointers + sizes, `stream` a
 * hipStream_t passed as void*, asynchronous on that stream, 0 on success and a negative RSU_E* code otherwise, returned before anything is
 * launched or written; no allocation, no host synchronisation). tests/test_gpu_thin_fenced.py holds every launching entry of this
 * header to the memory contract; road_segmentation_unet_amd/_lib.py binds it through its table SIGNATURES_THIN.
 */
#ifndef RSU_THIN_H_
#define RSU_THIN_H_

#include "rsu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- centre-lines (new; the reference has none) ----------------------------------------------------------------------------------- */
/* prob is float32 [N][H][W] (what the heads and predict() write), labels64 int64 [N][H][W]. The masks are rsu_distance.h's:
 *   images:   independent. Everything outside an image is background.
 *   counted:  a pixel is COUNTED iff its labels64 value is 0 or 1 (all 64 bits tested).
 *   P:        {counted and prob >= threshold}: one float32 comparison, the only float operation of this header. NaN is outside P,
 *             p == threshold is inside.
 *   T:        {labels64 == 1}. Ignored pixels are background for the thinning of both masks.
 *   rule:     Guo & Hall, CACM 32(3) 1989, algorithm A1. The neighbours of a pixel clockwise from north:
 *             p2 = N, p3 = NE, p4 = E, p5 = SE, p6 = S, p7 = SW, p8 = W, p9 = NW, and
 *               C = (!p2 & (p3|p4)) + (!p4 & (p5|p6)) + (!p6 & (p7|p8)) + (!p8 & (p9|p2))
 *               N = min((p9|p2) + (p3|p4) + (p5|p6) + (p7|p8), (p2|p3) + (p4|p5) + (p6|p7) + (p8|p9))
 *               m = (p6 | p7 | !p9) & p8 in sub-iteration 0, (p2 | p3 | !p5) & p4 in sub-iteration 1.
 *             A sub-iteration deletes every set pixel with C == 1, 2 <= N <= 3 and m == 0, all at once from the state before it. One
 *             ITERATION is sub-iteration 0 then 1; an iteration that deletes nothing is a fixed point. The skeleton is the mask after
 *             max_iters iterations or at its fixed point, whichever comes first: a function of the mask alone.
 *   limits:   N, H, W >= 1, H, W <= RSU_THIN_MAX_SIDE, 1 <= max_iters <= RSU_THIN_MAX_ITERS, threshold finite: RSU_EINVAL otherwise and
 *             for a NULL required pointer. RSU_E2BIG when prob, labels64 or an output reaches 0x7ffffff0 bytes (with labels64 or
 *             skel_true: N * H * W * 8).
 *
 * The method: both masks live in ws as bit rows, 64 - 4 K pixels to a 64-bit word (K = 8 whole iterations per launch: csrc/thin.h). An
 * init launch builds them from prob, threshold and labels64. Every step launch carries a tile -- one word wide, a workgroup's threads
 * high -- through K iterations in registers and LDS: a thread holds one row of the tile as ONE 64-bit word, the word's own pixels with
 * 2 K pixels of its neighbours to either side, and evaluates the rule bit-sliced, 64 pixels per operation (C and N as two-bit adders). A
 * sub-iteration looks one pixel out, so after 2 K of them the core of the tile is exact and the halo is dropped. A step launch adds the
 * pixels it deleted, per image and mask, to a counter of its own in ws (integer atomics, one per workgroup); the NEXT launch reads it
 * and returns at once for a mask that was already at its fixed point. A final launch writes the outputs and the counts. The launch count,
 * 2 + ceil(max_iters / K), is fixed by the arguments; no flag between workgroups, no grid-wide barrier, no float atomic: every result is
 * a function of the inputs alone.
 *
 * ws: rsu_thin_ws_bytes bytes, 8-byte aligned. It need not be cleared and holds nothing between calls. */
#define RSU_THIN_MAX_SIDE 1024
#define RSU_THIN_MAX_ITERS 512
size_t rsu_thin_ws_bytes(int N, int H, int W, int max_iters);   /* 0 for refused sizes */

/* skel_pred: float32 [N][H][W], 1.0 on the skeleton of P and 0.0 elsewhere.
 * skel_true: int64 [N][H][W], 1 on the skeleton of T and 0 on every other counted pixel; an ignored pixel keeps its labels64 value.
 * Either output may be NULL, not both. labels64 may be NULL iff skel_true is NULL: every pixel is then counted and T is empty.
 * acc:  may be NULL; otherwise unsigned 64-bit [4], ACCUMULATED (the caller zeroes it), and both outputs are required:
 *         acc[0] += |S_P|, acc[1] += |S_P and T|, acc[2] += |S_T|, acc[3] += |S_T and P|   (S_P, S_T the two skeletons)
 *       with one integer atomic add per non-zero counter per workgroup. An image without a counted pixel adds exactly nothing.
 * info: may be NULL; otherwise uint32 [N][2], WRITTEN: per image, for P ([n][0]) and T ([n][1]), the number of pixels the LAST executed
 *       iteration deleted. 0: converged within max_iters. Without labels64 [n][1] is 0.
 * Nothing is written outside skel_pred, skel_true, acc[0 .. 3], info and ws. */
/* align (rsu_mask_thin): prob 4, labels64 8, skel_pred 4, skel_true 8, acc 8, info 4, ws 8. */
int rsu_mask_thin(const float* prob, float threshold, const int64_t* labels64, int max_iters, float* skel_pred, int64_t* skel_true,
                  unsigned long long* acc, uint32_t* info, void* ws, int N, int H, int W, rsu_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RSU_THIN_H_ */
