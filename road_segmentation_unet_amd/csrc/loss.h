// loss.hip: the focal members of the opt-in head family (include/rsu_loss.h)
#pragma once
#include "elementwise.h"

// the focal training and evaluation heads (rsu_loss.h rsu_head_fwd_bwd_focal, rsu_head_eval_focal), gamma > 0 only: the grids and
// workspaces of ew_head_loss / ew_head_eval (elementwise.h), whose final kernels finish them
hipError_t ew_head_focal(const void* act, const float* w, const float* b, const int64_t* labels, const float* class_w, const float* pixel_w,
                         float gamma, const float* dice_sums, float dice_scale, float smooth, float* prob, void* dact, float* dw, float* db,
                         float* loss_sum, float* weight_sum, float* ws, long npix, int C, float inv_count, hipStream_t st);
hipError_t ew_head_eval_focal(const void* act, const float* w, const float* b, const int64_t* labels, const float* class_w, const float* pixel_w,
                              float gamma, float* prob, float* sums, unsigned long long* hist, float* ws, long npix, int C, hipStream_t st);
