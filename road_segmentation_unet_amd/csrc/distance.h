// Launch prototypes of the mask distance transform and its histogram (distance.hip; include/rsu_distance.h).
#pragma once
#include "rsu_common.h"

constexpr int DT_MAX_SIDE = 1024;   // largest H and W: a column is at most 16 chunks of 64 rows, a vertical distance fits 16 bits
constexpr int DT_BINS = 64;         // rsu_distance.h RSU_DIST_BINS
// one packed word of column distances per pixel
size_t dt_ws_bytes(int N, int H, int W);
// labels may be nullptr iff d2_true is (every pixel is then counted); either output may be nullptr
hipError_t dt_mask_distance(const float* prob, float threshold, const int64_t* labels, int32_t* d2_pred, int32_t* d2_true, void* ws, int N,
                            int H, int W, hipStream_t st);
hipError_t dt_distance_hist(const float* prob, float threshold, const int64_t* labels, unsigned long long* acc, void* ws, int N, int H, int W,
                            hipStream_t st);
