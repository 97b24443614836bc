// head.hip: the head of the net -- 1x1 conv (C -> 2) + softmax[..., 1] -- with every loss that is fused into it (rsu.h rsu_head_*,
// rsu_loss.h, rsu_cldice.h rsu_head_fwd_bwd_aux). One grid for all of them: ew_head_blocks() workgroups of 256 threads.
#pragma once
#include "rsu_common.h"

int ew_head_blocks(long npix, int C);
// the pinned pair: inference (train == false: labels, dact, dw, db, loss_sum, ws unused) and the unweighted training step (ws of
// ew_head_blocks() * (2 C + 3) floats)
hipError_t ew_head(bool train, const void* act, const float* w, const float* b, const int64_t* labels, float* prob, float* logits, void* dact, float* dw,
                   float* db, float* loss_sum, float* ws, long npix, int C, float inv_count, hipStream_t st);
// every other training head (rsu_head_fwd_bwd_w, _dice, _focal, _aux): ws of ew_head_blocks() * (2 C + 4) floats. Each term is chosen by
// its argument: gamma > 0 the focal modulation (gamma == 0: plain cross-entropy), dice_sums != nullptr the soft-Dice gradient from
// {I, P, Y} (else dice_scale and smooth are not read), gprob != nullptr a given d objective / d prob.
hipError_t hd_train(const void* act, const float* w, const float* b, const int64_t* labels, const float* class_w, const float* pixel_w, float gamma,
                    const float* dice_sums, float dice_scale, float smooth, const float* gprob, float* prob, void* dact, float* dw, float* db,
                    float* loss_sum, float* weight_sum, float* ws, long npix, int C, float inv_count, hipStream_t st);
// pass A of the soft-Dice head (rsu_head_dice_sums): forward only, ws of ew_head_blocks() * 3 floats
hipError_t ew_head_dice_sums(const void* act, const float* w, const float* b, const int64_t* labels, const float* pixel_w, float* prob,
                             float* dice_sums, float* ws, long npix, int C, hipStream_t st);
// the evaluation head (rsu_head_eval, rsu_head_eval_focal; gamma as above): forward only; ws of ew_head_eval_ws_floats() floats (5 partial
// sums and one 2 x EW_EVAL_BINS row of u32 counters per workgroup). EW_EVAL_BINS is rsu.h's RSU_EVAL_BINS.
constexpr int EW_EVAL_BINS = 256;
constexpr int EW_EVAL_SLICES = 8;   // k_head_eval_final: workgroups per 64-bin group (= adds per address of hist per call)
size_t ew_head_eval_ws_floats(long npix, int C);
hipError_t hd_eval(const void* act, const float* w, const float* b, const int64_t* labels, const float* class_w, const float* pixel_w, float gamma,
                   float* prob, float* sums, unsigned long long* hist, float* ws, long npix, int C, hipStream_t st);

// The sum of output o over the blocks' partials as every final kernel of the family forms it (k_cldice_final too): lane l adds partials
// l, l + 64, ... (independent loads), then a fixed-order butterfly. One wave per output.
static __device__ __forceinline__ float head_final_sum(const float* __restrict__ partial, int nblk, int nout, int o, int lane) {
    float t = 0.f;
    for (int bk = lane; bk < nblk; bk += 64) t += partial[(long)bk * nout + o];
    for (int m = 32; m > 0; m >>= 1) t += __shfl_xor(t, m);
    return t;
}
