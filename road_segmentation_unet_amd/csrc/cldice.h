// cldice.hip: the clDice term (include/rsu_cldice.h): the fused soft-skeleton forward and backward and the head that takes d objective / d prob
#pragma once
#include "elementwise.h"

constexpr int CL_MAX_ITERS = 16;   // rsu_cldice.h RSU_CLDICE_MAX_ITERS
constexpr int CL_FWD_TILE = 32;    // the forward's tile side: one workgroup per tile, one row of four partial sums per workgroup
// workgroups of the forward launch (= rows of partial sums in ws)
long cl_fwd_tiles(int B, int H, int W);
// ws: (2 iters + 1) maps of B H W floats -- E_1 .. E_{iters+1} and S_0 .. S_{iters-1} of the prob map, which the backward reads -- and behind
// them cl_fwd_tiles() * 4 partial sums
size_t cl_ws_floats(int B, int H, int W, int iters);
hipError_t cl_fwd(const float* prob, const int64_t* labels, int iters, float* skel_p, float* skel_y, float* sums, float* ws, int B, int H, int W,
                  hipStream_t st);
hipError_t cl_bwd(const float* prob, const int64_t* labels, const float* skel_y, const float* sums, int iters, float scale, float smooth,
                  float* gprob, const float* ws, int B, int H, int W, hipStream_t st);
// the training head with a given d objective / d prob (rsu_head_fwd_bwd_aux): ew_head_loss's / ew_head_focal's grid, workspace and final
// kernel; gamma == 0 takes the cross-entropy lines of k_head_loss
hipError_t cl_head_aux(const void* act, const float* w, const float* b, const int64_t* labels, const float* class_w, const float* pixel_w,
                       float gamma, const float* dice_sums, float dice_scale, float smooth, const float* gprob, float* prob, void* dact, float* dw,
                       float* db, float* loss_sum, float* weight_sum, float* ws, long npix, int C, float inv_count, hipStream_t st);
