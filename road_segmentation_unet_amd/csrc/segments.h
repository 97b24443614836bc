// Launch prototypes of the road-segment extraction (segments.hip; include/rsu_segments.h).
#pragma once
#include "rsu_common.h"

constexpr int SG_MAX_SIDE = 1024;     // largest H and W
constexpr int SG_MAX_EDGES = 65536;   // largest max_edges
// ws: the four float32 mask planes [4 N][H][W] (S_P, S_T, Z_P, Z_T), three int32 arrays of the same shape (the labels; the labelling's
// parents, which hold the roots' ranks afterwards; its per-root totals), then the compaction's block counts [4 N][ceil(H W / SG_BLOCK)]
size_t sg_ws_bytes(int N, int H, int W);
// the launches of one call: classify, the labelling's 2 + cc_levels(H, W), count, scan, place, measure, finish
int sg_launches(int H, int W);
// labels may be nullptr iff every *_true pointer is (every pixel is then counted, T is empty); seg_*, node_* and acc may be nullptr
hipError_t sg_line_segments(const float* prob, float threshold, const int64_t* labels, int max_edges, int32_t* edges_pred, int32_t* edges_true,
                            int32_t* counts, int32_t* seg_pred, int32_t* seg_true, int32_t* node_pred, int32_t* node_true,
                            unsigned long long* acc, void* ws, int N, int H, int W, hipStream_t st);
