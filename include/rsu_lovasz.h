/*
 * rsu_lovasz.h -- the fifth public header of librsu_hip.so: the Lovasz (Jaccard surrogate) loss term with a device-side sort.
 *
 * Same library, same conventions and memory contract as rsu.h (plain C, device pointers + sizes, `stream` a hipStream_t passed as void*,
 * asynchronous on that stream, 0 on success and a negative RSU_E* code otherwise). tests/test_gpu_lovasz_fenced.py holds every launching
 * entry of this header to the memory contract; road_segmentation_unet_amd/_lib.py binds it through its table SIGNATURES_LOVASZ.
 */
#ifndef RSU_LOVASZ_H_
#define RSU_LOVASZ_H_

#include "rsu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- the Lovasz hinge on probabilities (new; the reference has none): Berman, Triki and Blaschko, CVPR 2018 -------- */
/* The Lovasz extension of the Jaccard loss: a convex surrogate of 1 - IoU per image, the figure every validation pass prints. All
 * float32 unless stated. p = prob [B][H][W] (what the heads write), labels int64 [B][H][W]. A pixel is COUNTED when its label is 0 or 1
 * (all 64 bits tested), y is that label. Images are independent: no order, count or sum crosses from one image into another.
 * For image b with n counted pixels, G of them at y = 1:
 *   e_i  = fabsf(f32(y_i) - p_i)                          (one subtraction, the sign cleared: the bit pattern is below 2^31)
 *   order: counted pixels by the UNSIGNED 32-BIT PATTERN of e_i, descending; ties by ascending row-major pixel index. A total order:
 *          NaN, infinities and values outside [0, 1] sort where their bits fall. r(i) in 1..n is the rank of pixel i.
 *   c_k  = the number of y = 1 pixels among ranks 1..k    (an integer)
 *   I_k  = G - c_k, U_k = G + k - c_k (>= 1), both converted to float32 exactly (H * W <= 2^24)
 *   J_0  = 0, J_k = 1 - I_k / U_k                         (one correctly rounded division, one subtraction)
 *   g_k  = J_k - J_{k-1}                                  (one subtraction)
 *   L_b  = sum_k e_{pi(k)} * g_k                          (one multiplication each; the order of the sum is given below); 0 when n = 0
 * G = 0 gives g_1 = 1 and every other g_k = 0: the loss is the largest error. The term is scale * (1 / B) * sum_b L_b, B the call's B
 * (images without a counted pixel included). Gradient wrt p, with c = f32(scale) / f32(B) (one division): c * g_{r(i)} (one
 * multiplication), negated where y_i = 1; +0 at an ignored pixel, whose p is not looked at. accumulate != 0: the value is ADDED to what
 * gprob holds (one rounding); otherwise it overwrites. hostio.lovasz_loss / hostio.lovasz_gradient restate all of it.
 *
 * The sort: a bitonic network over unique 64-bit keys (bits(e) << 32 | a counted flag | (2^24 - 1 - index) << 1 | y), every image padded
 * with zero keys to Pn = max(4096, the next power of two >= H * W); ignored pixels are zero keys as well, so the n counted pixels come
 * first. Tiles of 4096 keys are sorted and merged in LDS; the compare-exchange steps of stride >= 4096 run through global memory, up to
 * three steps per launch in registers. With q = log2(Pn) - 12 the sort is 1 + q + sum_{m=1..q} ceil(m / 3) launches; one more launch scans
 * y along the ranks, forms J_k, g_k and the products, sums each tile's products and scatters the gradient; a last one adds the tiles'
 * sums. The launch count depends on B, H, W alone, never on the data: q + 3 + sum_{m=1..q} ceil(m / 3) -- 3 for H * W <= 4096, 18 at 388 x 388.
 * No grid-wide barrier, no cooperative launch, no flag between workgroups, no atomic of any kind. The order of L_b's sum: a thread adds
 * its 8 consecutive ranks in order, the 512 threads of a tile are added by a binary tree (halving strides); of an image's tiles thread i
 * of 256 adds tiles i, i + 256, .. in order and the same tree adds the threads; sum_b L_b in order of b. The bits are the same on every run.
 *
 * rsu_lovasz_fwd: loss_sum[0] += sum_b L_b, loss_sum[1] += B (the caller zeroes them). The evaluation's entry.
 * rsu_lovasz_fwd_bwd: the same, and gprob [B][H][W] written or accumulated as above.
 * ws: rsu_lovasz_ws_bytes bytes, 8-byte aligned: B * Pn keys of 8 bytes and, per tile of 4096 keys, two int32 counts and one float sum.
 * It need not be cleared and holds nothing between calls.
 * No host synchronisation; nothing is written outside gprob, loss_sum[0..1] and ws. Errors, returned before anything is launched or
 * written: RSU_EINVAL for a NULL pointer, B, H, W < 1, H * W > 2^24, B * H * W >= 2^31, a scale that is not finite and >= 0. */
size_t rsu_lovasz_ws_bytes(int B, int H, int W);   /* 0 for refused arguments */
/* align (rsu_lovasz_fwd): prob 4, labels 8, loss_sum 4, ws 8. */
int rsu_lovasz_fwd(const float* prob, const int64_t* labels, float* loss_sum, void* ws, int B, int H, int W, rsu_stream_t stream);
/* align (rsu_lovasz_fwd_bwd): prob 4, labels 8, gprob 4, loss_sum 4, ws 8. */
int rsu_lovasz_fwd_bwd(const float* prob, const int64_t* labels, float scale, int accumulate, float* gprob, float* loss_sum, void* ws, int B,
                       int H, int W, rsu_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RSU_LOVASZ_H_ */
