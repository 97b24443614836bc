// Launch prototypes of the mask thinning (thin.hip; include/rsu_thin.h).
#pragma once
#include "rsu_common.h"

// whole iterations per step launch: the halo of a tile is 2 * TH_K pixels (tools/bench_thin.py times 2, 4 and 8 from A/B builds:
// make VARIANT=thinK EXTRA=-DTH_K=K; profiles/r24/thin.txt)
#ifndef TH_K
#define TH_K 8
#endif
constexpr int TH_MAX_SIDE = 1024;   // largest H and W
constexpr int TH_MAX_ITERS = 512;
constexpr int TH_HALO = 2 * TH_K;
constexpr int TH_CORE = 64 - 2 * TH_HALO;   // pixels per 64-bit word of a bit row in ws
static_assert(TH_K >= 1 && TH_K <= 8, "a 64-bit window needs a core");
// three bit planes (the masks; two working copies) of [N][2][H][ceil(W / TH_CORE)] words, then the counters
size_t th_ws_bytes(int N, int H, int W, int max_iters);
// labels may be nullptr iff skel_true is (every pixel is then counted, T is empty); either output may be nullptr; acc and info may be
hipError_t th_mask_thin(const float* prob, float threshold, const int64_t* labels, int max_iters, float* skel_pred, int64_t* skel_true,
                        unsigned long long* acc, uint32_t* info, void* ws, int N, int H, int W, hipStream_t st);
