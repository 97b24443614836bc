// Launch prototypes of the centre-line pruning and node classification (graph.hip; include/rsu_graph.h).
#pragma once
#include "rsu_common.h"

// prune / regrow rounds per step launch: a round looks one pixel out, so the halo of a tile is GR_R pixels (tools/bench_graph.py times
// 4, 8 and 16 from A/B builds: make VARIANT=graphR EXTRA=-DGR_R=R; profiles/r25/graph.txt)
#ifndef GR_R
#define GR_R 16
#endif
constexpr int GR_MAX_SIDE = 1024;   // largest H and W
constexpr int GR_MAX_BRANCH = 64;
constexpr int GR_HALO = GR_R;
constexpr int GR_CORE = 64 - 2 * GR_HALO;   // pixels per 64-bit word of a bit row in ws
static_assert(GR_R >= 2 && GR_R <= 16, "a 64-bit window needs a core, and the first regrow launch a round behind END(X1)");
// min_branch == 0: one bit plane [N][2][H][ceil(W / GR_CORE)] of words (the masks). Otherwise five (the masks; two working copies of the
// delete phase; two of the regrow phase), then the counters [ceil(L / GR_R) + ceil((L + 1) / GR_R)][N][2]
size_t gr_ws_bytes(int N, int H, int W, int min_branch);
// labels may be nullptr iff out_true and junc_true are (every pixel is then counted, T is empty); every output may be nullptr, acc too
hipError_t gr_skeleton_graph(const float* prob, float threshold, const int64_t* labels, int min_branch, float* out_pred, int64_t* out_true,
                             float* junc_pred, int64_t* junc_true, unsigned long long* acc, void* ws, int N, int H, int W, hipStream_t st);
