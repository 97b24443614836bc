// lovasz.hip: the Lovasz (Jaccard surrogate) term (include/rsu_lovasz.h): a bitonic sort of every image's errors, the scan along the ranks,
// the Jaccard differences, the loss and the gradient scattered back to the pixels
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

constexpr int LV_TILE = 4096;          // keys per LDS tile: one workgroup of 512 threads, 8 consecutive keys per thread
constexpr int LV_MAX_PIXELS = 1 << 24; // H * W: the integers I_k, U_k are exact in float32, and a pixel index fits its 24 key bits
// the padded length of an image's key segment: max(LV_TILE, the next power of two >= H * W)
long lv_padded(int H, int W);
// ws: B * lv_padded keys of 8 bytes, then per tile two int32 counts {y = 1, counted}, then per tile one float sum of products
size_t lv_ws_bytes(int B, int H, int W);
// gprob == nullptr: the forward alone. c = f32(scale) / f32(B), formed by the caller.
hipError_t lv_run(const float* prob, const int64_t* labels, float c, int accumulate, float* gprob, float* loss_sum, void* ws, int B, int H,
                  int W, hipStream_t st);
