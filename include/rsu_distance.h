/*
 * rsu_distance.h -- the seventh public header of librsu_hip.so: the exact squared Euclidean distance from every pixel to a predicted mask
 * and to a truth mask, on the device, and the one-pass reduction of those distances to a histogram from which the host reads the
 * buffer-relaxed precision, recall and F1 of Mnih & Hinton at every slack at once.
 *
 * Same library, same conventions and memory contract as rsu.h and rsu_components.h (plain C, device pointers + sizes, `stream` a
 * hipStream_t passed as void*, asynchronous on that stream, 0 on success and a negative RSU_E* code otherwise, returned before anything is
 * launched or written; no allocation, no host synchronisation). tests/test_gpu_distance_fenced.py holds every launching entry of this
 * header to the memory contract; road_segmentation_unet_amd/_lib.py binds it through its table SIGNATURES_DISTANCE.
 */
#ifndef RSU_DISTANCE_H_
#define RSU_DISTANCE_H_

#include "rsu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- mask distances (new; the reference has none) -------------------------------------------------------------------------------- */
/* Shared by both entries. prob is float32 [N][H][W] (what the heads and predict() write), labels64 int64 [N][H][W].
 *   images:   independent. No distance crosses from one image into the next.
 *   counted:  a pixel is COUNTED iff its labels64 value is 0 or 1 (all 64 bits tested, as in the heads and in rsu_components_pair_count).
 *   P:        {counted and prob >= threshold}: one float32 comparison, the only float operation of this header. NaN is outside P,
 *             p == threshold is inside (the rule of rsu_quantize_mask).
 *   T:        {labels64 == 1}.
 *   D2_M(q):  min over m in M of (qy - my)^2 + (qx - mx)^2, in exact integers; RSU_DIST_NONE when M is empty in that image. Ignored
 *             pixels are plain geometry: distances run across them.
 *   bin(d2):  min(r, RSU_DIST_BINS - 1), r the smallest integer with r * r >= d2; RSU_DIST_NONE maps to the last bin. Integer-only, so
 *             d2 <= rho^2 iff bin <= rho for rho <= RSU_DIST_BINS - 2.
 *   limits:   N, H, W >= 1, H, W <= RSU_DIST_MAX_SIDE, threshold finite: RSU_EINVAL otherwise and for a NULL required pointer.
 *             RSU_E2BIG when prob, labels64 or an output reaches 0x7ffffff0 bytes (with labels64: N * H * W * 8).
 *
 * The method: the separable transform in integer arithmetic. A column launch builds both masks from prob, threshold and labels64 (64 rows
 * per thread as two 64-bit words, bit scans inside the chunk, carries through LDS) and writes one packed word per pixel into ws: the
 * vertical distances to T (low 16 bits) and to P (high 16 bits), 0xffff = none in this column. A row launch stages the squared column
 * distances in LDS and scans outwards from each pixel until d * d reaches the best found so far. Two launches per call, a count fixed by
 * the arguments. No global atomic per pixel, no float atomic, no grid-wide barrier, no flag between workgroups: the histogram is counted
 * with LDS integer atomics and flushed with one 64-bit integer atomic add per non-zero bin per workgroup, so every result is a function of
 * the inputs alone.
 *
 * ws: rsu_distance_ws_bytes bytes = 4 * N * H * W, 4-byte aligned. It need not be cleared and holds nothing between calls. */
#define RSU_DIST_BINS 64
#define RSU_DIST_NONE 0x7fffffff
#define RSU_DIST_MAX_SIDE 1024
size_t rsu_distance_ws_bytes(int N, int H, int W);          /* 0 for refused sizes */

/* exact squared distances. d2_pred[q] = D2_P(q), d2_true[q] = D2_T(q), int32 [N][H][W], at EVERY pixel (ignored ones included).
 * Either output may be NULL, not both. labels64 may be NULL iff d2_true is NULL: every pixel is then counted.
 * Nothing is written outside d2_pred, d2_true and ws. */
/* align (rsu_mask_distance): prob 4, labels64 8, d2_pred 4, d2_true 4, ws 4. */
int rsu_mask_distance(const float* prob, float threshold, const int64_t* labels64, int32_t* d2_pred, int32_t* d2_true,
                      void* ws, int N, int H, int W, rsu_stream_t stream);

/* acc: unsigned 64-bit [2][RSU_DIST_BINS], ACCUMULATED (the caller zeroes it):
 *   acc[0][b] += #{q in P : bin(D2_T(q)) == b}      (predicted pixels by their distance to the truth)
 *   acc[1][b] += #{q in T : bin(D2_P(q)) == b}      (true pixels by their distance to the prediction)
 * An image without a counted pixel (the padding of an evaluation chunk: labels -1) has P and T empty and adds exactly nothing. The row
 * scan stops at d = RSU_DIST_BINS - 2: nothing past the last bin is needed, which bounds its cost whatever the data.
 * Nothing is written outside acc[0 .. 2 * RSU_DIST_BINS - 1] and ws. */
/* align (rsu_distance_hist): prob 4, labels64 8, acc 8, ws 4. */
int rsu_distance_hist(const float* prob, float threshold, const int64_t* labels64, unsigned long long* acc,
                      void* ws, int N, int H, int W, rsu_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RSU_DISTANCE_H_ */
