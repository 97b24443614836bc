// cldice.hip: the clDice term (include/rsu_cldice.h): the fused soft-skeleton forward and backward. (The head that takes their
// d objective / d prob, rsu_head_fwd_bwd_aux, is head.hip's hd_train.)
#pragma once
#include "head.h"   // head_final_sum: k_cldice_final sums the tiles' partials as the heads' final kernels do

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
