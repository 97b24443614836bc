// The separable exact squared Euclidean distance transform of two masks at once, shared by distance.hip and border_map.hip. Integer
// code only: both owners are built with -ffp-contract=off and keep every float operation in their own files.
//
// Column pass: threads across x, one wave per 64 rows of a 64-column strip, block (64, ceil(H / 64)). A thread builds both masks of
// its 64 rows in registers (the owner's loop) and calls edt_cols_store: the nearest mask pixel at or above and at or below every row is a
// bit scan inside the chunk plus one carry per direction from the other chunks of the column, handed over through LDS. One word per
// pixel: g0 | g1 << 16, the vertical distances to mask 0 / mask 1 (0 = the pixel itself; EDT_NONE = the column has none).
// Row pass: one workgroup per row stages the squares of both (edt_stage), every thread takes min over x' of (x - x')^2 + g(x')^2,
// scanning outwards and stopping once (x - x')^2 alone reaches the minimum so far (edt_scan).
#pragma once
#include "rsu_common.h"

constexpr int EDT_BIG = 0x40000000;      // "no mask pixel in the column", as a square: EDT_BIG + 1023^2 stays below 2^31
constexpr unsigned EDT_NONE = 0xffffu;   // the same in a packed word
constexpr int EDT_ABOVE = -0x20000, EDT_BELOW = 0x40000;   // row numbers of "none above" / "none below": any distance to them is > 0xffff

// m0, m1: the masks of rows y0 .. y0 + 63 (y0 = 64 * threadIdx.y) of column x, 0 past the image; lds: int [4][blockDim.y][64]; img: the
// offset of the image in ws. Every thread of the workgroup calls it (it holds a barrier)
__device__ __forceinline__ void edt_cols_store(unsigned long long m0, unsigned long long m1, int* lds, uint32_t* __restrict__ ws, size_t img,
                                               int x, int H, int W) {
    const int tx = threadIdx.x, k = threadIdx.y, CH = blockDim.y, y0 = k * 64;
    int* last0 = lds;
    int* last1 = last0 + CH * 64;
    int* first0 = last1 + CH * 64;
    int* first1 = first0 + CH * 64;
    const int slot = k * 64 + tx;
    last0[slot] = m0 ? y0 + 63 - __clzll((long long)m0) : EDT_ABOVE;
    last1[slot] = m1 ? y0 + 63 - __clzll((long long)m1) : EDT_ABOVE;
    first0[slot] = m0 ? y0 + __ffsll((long long)m0) - 1 : EDT_BELOW;
    first1[slot] = m1 ? y0 + __ffsll((long long)m1) - 1 : EDT_BELOW;
    __syncthreads();
    int up0 = EDT_ABOVE, up1 = EDT_ABOVE, dn0 = EDT_BELOW, dn1 = EDT_BELOW;
    for (int kk = 0; kk < k; ++kk) {
        up0 = max(up0, last0[kk * 64 + tx]);
        up1 = max(up1, last1[kk * 64 + tx]);
    }
    for (int kk = k + 1; kk < CH; ++kk) {
        dn0 = min(dn0, first0[kk * 64 + tx]);
        dn1 = min(dn1, first1[kk * 64 + tx]);
    }
    if (x >= W) return;
    const int rows = min(64, H - y0);
    for (int i = 0; i < rows; ++i) {
        const int y = y0 + i;
        const unsigned long long upto = ~0ull >> (63 - i);
        const unsigned long long lo0 = m0 & upto, lo1 = m1 & upto, hi0 = m0 >> i, hi1 = m1 >> i;
        const int a0 = lo0 ? y0 + 63 - __clzll((long long)lo0) : up0, b0 = hi0 ? y + __ffsll((long long)hi0) - 1 : dn0;
        const int a1 = lo1 ? y0 + 63 - __clzll((long long)lo1) : up1, b1 = hi1 ? y + __ffsll((long long)hi1) - 1 : dn1;
        const unsigned g0 = (unsigned)min(min(y - a0, b0 - y), (int)EDT_NONE);
        const unsigned g1 = (unsigned)min(min(y - a1, b1 - y), (int)EDT_NONE);
        ws[img + (size_t)y * W + x] = g0 | (g1 << 16);
    }
}

// the squares of a row's packed column distances to lds as int [2][Wp] (EDT_NONE -> EDT_BIG). Returns bit c: some column of the row has
// a pixel of mask c. Every thread of the workgroup calls it: it ends in the barrier behind the staging. nthreads: blockDim.x, read by
// the kernel itself (read in here, the reduction behind it derives the workgroup's size from the grid's with two dependent loads)
__device__ __forceinline__ int edt_stage(const uint32_t* __restrict__ ws, size_t row, int* lds, int W, int Wp, int nthreads) {
    int any = 0;
    for (int x = threadIdx.x; x < W; x += nthreads) {
        const unsigned u = ws[row + x];
        const int g0 = (int)(u & 0xffffu), g1 = (int)(u >> 16);
        lds[x] = g0 == (int)EDT_NONE ? EDT_BIG : g0 * g0;
        lds[Wp + x] = g1 == (int)EDT_NONE ? EDT_BIG : g1 * g1;
        any |= (g0 != (int)EDT_NONE ? 1 : 0) | (g1 != (int)EDT_NONE ? 2 : 0);
    }
    return (__syncthreads_or(any & 1) ? 1 : 0) | (__syncthreads_or(any & 2) ? 2 : 0);
}

// min over x' of (x - x')^2 + g2[x'] along a staged row of W squares; scan false: g2[x] alone (no column of the row has a mask pixel)
template <class T>
__device__ __forceinline__ int edt_scan(const T* g2, int x, int W, bool scan = true) {
    int best = g2[x];
    if (scan) {
        const int dmax = max(x, W - 1 - x);
        // (a clamped index re-reads the edge column with a larger d: never below what that column already gave)
        for (int d = 1; d <= dmax && d * d < best; ++d) best = min(best, min((int)g2[max(x - d, 0)], (int)g2[min(x + d, W - 1)]) + d * d);
    }
    return best;
}
