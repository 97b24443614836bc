/*
 * rsu_loss.h -- the third public header of librsu_hip.so: loss entries added behind rsu.h (the focal cross-entropy heads).
 *
 * Same library, same conventions and memory contract as rsu.h (plain C, device pointers + sizes, `stream` a hipStream_t passed as void*,
 * asynchronous on that stream, 0 on success and a negative RSU_E* code otherwise). tests/test_gpu_loss_fenced.py holds every launching
 * entry of this header to the memory contract, as tests/test_gpu_fenced.py does for rsu.h; road_segmentation_unet_amd/_lib.py binds it
 * through its table SIGNATURES_LOSS.
 */
#ifndef RSU_LOSS_H_
#define RSU_LOSS_H_

#include "rsu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- focal cross-entropy (new; the reference has none): Lin et al. 2017, on the heads of rsu.h -------- */
/* rsu_head_fwd_bwd_w / rsu_head_fwd_bwd_dice / rsu_head_eval (rsu.h) with every counted pixel's cross-entropy scaled by how wrong the
 * network is on it. Per pixel p whose label is 0 or 1 (tested on all 64 bits; any other label IGNORES the pixel by selection, as in
 * those entries: a +0 dact row, nothing added to any sum, whatever its pixel_w holds), float32:
 *   t = label, o = 1 - t;  p_t, p_o the two softmax outputs (the expressions of the other heads: prob gets their bits)
 *   CE     = -(l_t - m - log s),  m = max(l_0, l_1), s = exp(l_0 - m) + exp(l_1 - m)
 *   omega  = class_w[t] * pixel_w[p]                      (class_w NULL: (1, 1); pixel_w NULL: all 1)
 *   F      = p_o ^ gamma = exp2(gamma * log2(p_o))        (the modulating factor (1 - p_t)^gamma, from p_o: no cancellation)
 *   loss_p = omega * F * CE
 *   g      = omega * inv_count * F * (p_o + gamma * p_t * CE);   dlogit[t] = -g,  dlogit[o] = +g
 * (d/dz_t [-p_o^gamma log p_t] = p_o^gamma (gamma p_t log p_t - p_o); with gamma = 0 the cross-entropy gradient p_t - 1). No division.
 * Corners: p_o == 0 gives gamma * -inf = -inf, exp2(-inf) = 0: loss_p = 0, g = 0. p_t == 0 leaves CE finite (its log-sum-exp form),
 * p_t * CE = 0 and F = 1: g = omega * inv_count. No output is NaN or inf for finite inputs.
 * inv_count stays 1 / (global pixel count): nothing is renormalised by sum F (no second pass; a SUM all-reduce of the gradients and of
 * loss_sum stays correct). The gradient is smaller than the cross-entropy's, so a learning rate tuned for gamma = 0 is not tuned here.
 *
 * rsu_head_fwd_bwd_focal: the training head. += loss_sum[0] receives sum omega F CE and weight_sum[0] (may be NULL) sum omega -- the
 * caller zeroes both, as for rsu_head_fwd_bwd_w; prob [npix], dact [npix][C] bf16 (through the ReLU in front of the head), dw [C][2] and
 * db [2] are overwritten. ws: rsu_head_dice_ws_floats(npix, C) floats. It need not be cleared and holds nothing between calls (the Dice
 * sums of pass A arrive in dice_sums, not in ws).
 *   dice_sums == NULL: the focal head alone; dice_scale and smooth are not looked at.
 *   dice_sums != NULL: pass B of the soft-Dice head behind an unchanged rsu_head_dice_sums: the Dice gradient of rsu_head_fwd_bwd_dice is
 *   added to dlogit exactly as there (neither the class weights nor F enter it); dice_sums is read only.
 * rsu_head_eval_focal: the evaluation head, rsu_head_eval with sums[0] += sum omega F CE: sums[1..4] += {sum omega, I, P, Y} and hist
 * [2][RSU_EVAL_BINS] receive what rsu_head_eval adds, bit for bit; the caller zeroes the accumulators before the first batch.
 * ws: rsu_head_eval_ws_floats(npix, C) floats. It need not be cleared and holds nothing between calls. From zeroed accumulators sums[0] has the bits of the training entry's loss_sum.
 * gamma == 0 is decided on the host: the call launches exactly what rsu_head_fwd_bwd_w / rsu_head_fwd_bwd_dice / rsu_head_eval launch.
 * Errors, returned before anything is launched or written: RSU_EINVAL for a gamma that is not finite or is negative, and for whatever
 * the corresponding entry of rsu.h refuses (a NULL among act, w, b, labels, prob, loss_sum / sums, hist, dact, dw, db, ws; a C that is
 * not 8 * 2^k in [8, 512]; npix < 1; with dice_sums != NULL a smooth that is not finite and > 0 or a dice_scale that is not finite
 * and >= 0). */
/* align (rsu_head_fwd_bwd_focal): act 16, w 4, b 4, labels 8, class_w 4, pixel_w 4, dice_sums 4, prob 4, loss_sum 4, weight_sum 4, dact 16, dw 4,
 * db 4, ws 4. */
int rsu_head_fwd_bwd_focal(const void* act, const float* w, const float* b, const int64_t* labels, const float* class_w /* may be NULL */,
                           const float* pixel_w /* may be NULL */, float gamma, const float* dice_sums /* may be NULL */, float dice_scale,
                           float smooth, float* prob, float* loss_sum, float* weight_sum /* may be NULL */, void* dact, float* dw, float* db,
                           float* ws, long npix, int C, float inv_count, rsu_stream_t stream);
/* align (rsu_head_eval_focal): act 16, w 4, b 4, labels 8, class_w 4, pixel_w 4, prob 4, sums 4, hist 8, ws 4. */
int rsu_head_eval_focal(const void* act, const float* w, const float* b, const int64_t* labels, const float* class_w /* may be NULL */,
                        const float* pixel_w /* may be NULL */, float gamma, float* prob, float* sums, unsigned long long* hist, float* ws,
                        long npix, int C, rsu_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RSU_LOSS_H_ */
