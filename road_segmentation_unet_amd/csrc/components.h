// components.hip: connected-component labelling of binary masks (include/rsu_components.h): union-find per 64 x 64 tile in LDS, a
// hierarchy of border merges in which every set belongs to one workgroup, a flatten and a gather launch
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

constexpr int CC_TILE = 64;             // the tile's side: a row of a tile is one wave's ballot
constexpr int CC_MAX_PIXELS = 1 << 24;  // H * W: an area fits the 25 low bits of a total, the edge flag sits at bit 30
// a per-root total (cc_label leaves them behind the parents in ws): the area in the low bits, the edge flag above (segments.hip reads the area)
constexpr int CC_EDGE = 1 << 30;
constexpr int CC_AREA = (1 << 25) - 1;
static_assert(CC_MAX_PIXELS <= CC_AREA, "an area fits below the edge flag");
// the merge launches of one labelling: ceil(log2(max(tiles_y, tiles_x)))
int cc_levels(int H, int W);
// ws: five int32 arrays of N * H * W elements and four int32 counters per image
size_t cc_ws_bytes(int N, int H, int W);
// labels doubles as the tile-area array until the flatten launch overwrites it; area and edge may be nullptr
hipError_t cc_label(const float* prob, float threshold, int connectivity, int invert, int32_t* labels, int32_t* area, uint8_t* edge, void* ws,
                    int N, int H, int W, hipStream_t st);
hipError_t cc_filter(const float* prob, float threshold, int connectivity, int min_area, int max_hole, float* out, int64_t* stats, void* ws,
                     int N, int H, int W, hipStream_t st);
hipError_t cc_pair_count(const float* prob, float threshold, const int64_t* labels64, int connectivity, unsigned long long* acc, void* ws, int N,
                         int H, int W, hipStream_t st);
