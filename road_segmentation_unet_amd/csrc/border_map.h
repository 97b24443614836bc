// Launch prototypes of the border-distance weight map (border_map.hip; rsu.h rsu_border_map).
#pragma once
#include "rsu_common.h"

constexpr int BM_MAX_SIDE = 1024;   // largest H and W the staging holds (rsu.h states the range)
// one packed word of column distances per pixel
size_t bm_ws_bytes(int N, int H, int W);
hipError_t bm_border_map(const int64_t* labels, const float* mul, float* out, int32_t* d2, void* ws, int N, int H, int W, float w0,
                         float neg_inv_2s2, hipStream_t st);
