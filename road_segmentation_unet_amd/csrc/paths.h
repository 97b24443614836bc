// Launch prototypes of the segment ordering (paths.hip; include/rsu_paths.h).
#pragma once
#include "rsu_common.h"

constexpr int PT_MAX_SIDE = 1024;       // largest H and W
constexpr int PT_MAX_EDGES = 65536;     // largest max_edges
constexpr int PT_MAX_LEN = 1 << 20;     // largest max_len
// the doublings of one call: ceil(log2(max_len))
int pt_rounds(int max_len);
// ws: two arc buffers of 64-bit words [N][H][W][2], the pixel plane int32 [N][H][W] (row << 8 | link mask, or -1), the rows' smallest
// terminals and branched flags int32 [N][max_edges] each, then the changed-arc counts int32 [max(R, 1)][N], R = pt_rounds(max_len)
size_t pt_ws_bytes(int N, int H, int W, int max_edges, int max_len);
// the launches of one call: init, classify, rows, arcs, R jumps, emit
int pt_launches(int max_len);
// pos may be nullptr
hipError_t pt_segment_paths(const int32_t* seg, const int32_t* edges, const int32_t* counts, int side, int max_edges, int max_len, int max_points,
                            int32_t* paths, int32_t* offsets, int32_t* kind, int32_t* pos, int32_t* info, void* ws, int N, int H, int W,
                            hipStream_t st);
