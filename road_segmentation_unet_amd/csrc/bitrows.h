// Bit rows, shared by the mask tools that work on them (thin.hip, graph.hip): the layout of a bit plane, the launch that builds the planes
// and the tile of a step launch. Integer code but for one comparison. Every piece is a template on its owner's constants: CORE and HALO
// differ between the owners as soon as one of them is built with another TH_K or GR_R.
//
// A plane is [N][2][H][Wq] 64-bit words (side 0 = P = {counted and prob >= threshold}, side 1 = T = {label == 1}), Wq = ceil(W / CORE): a
// word keeps CORE pixels of a row in its low bits (bit i = pixel xw * CORE + i), the bits above and the pixels past W stay 0. A step tile
// is one workgroup of ROWS threads per image side, row tile and word column; a thread holds ONE 64-bit window of one row -- HALO pixels
// of the word to the left, the word's CORE pixels, HALO pixels of the word to the right -- and hands it to its neighbours through LDS.
#pragma once
#include "rsu_common.h"

namespace bitrows {

typedef unsigned long long u64;

template <int CORE>
inline int wq(int W) { return (W + CORE - 1) / CORE; }
template <int CORE>
inline size_t plane_words(int N, int H, int W) { return (size_t)N * 2 * H * wq<CORE>(W); }
// the bytes of `count` 32-bit counters behind the planes, rounded up to whole words
inline size_t counter_bytes(size_t count) { return (count * sizeof(uint32_t) + 7) / 8 * 8; }

// The body of an init launch: grid N * H (one workgroup per image row), block THREADS. Coalesced label and probability loads, one ballot
// per wave and mask into LDS as plain 64-pixel words, then one thread per plane word cuts its CORE pixels out. Writes plane_o and, where
// given, plane_x; clears the image's own counters, two per launch that has some. LAB: labels given (else every pixel counted, T empty)
template <bool LAB, int CORE, int THREADS, int MAX_SIDE>
__device__ __forceinline__ void init_row(const float* __restrict__ prob, float threshold, const int64_t* __restrict__ labels,
                                         u64* __restrict__ plane_o, u64* __restrict__ plane_x, uint32_t* __restrict__ counters, int nlaunch,
                                         int N, int H, int W, int Wq) {
    __shared__ u64 bits[2][MAX_SIDE / 64 + THREADS / 64 + 1];   // (a wave past W still stores its empty ballot)
    const int n = blockIdx.x / H, y = blockIdx.x - n * H, tid = threadIdx.x;
    if (y == 0)
        for (int i = tid; i < 2 * nlaunch; i += THREADS) counters[((size_t)(i >> 1) * N + n) * 2 + (i & 1)] = 0;
    for (int i = tid; i < 2 * (int)(sizeof(bits[0]) / sizeof(u64)); i += THREADS) (&bits[0][0])[i] = 0;
    __syncthreads();
    const size_t row = ((size_t)n * H + y) * W;
    for (int x0 = 0; x0 < W; x0 += THREADS) {
        const int x = x0 + tid;
        const bool in = x < W;
        const size_t at = row + (in ? x : W - 1);   // (lanes past the row load a valid address and drop the value)
        const int64_t l = LAB ? labels[at] : 0;
        const float p = prob[at];
        const bool counted = l == 0 || l == 1;
        const u64 mp = __ballot(in && counted && p >= threshold);   // (NaN compares false)
        const u64 mt = __ballot(LAB && in && l == 1);
        if ((tid & 63) == 0) {
            bits[0][x >> 6] = mp;
            bits[1][x >> 6] = mt;
        }
    }
    __syncthreads();
    for (int i = tid; i < 2 * Wq; i += THREADS) {
        const int side = i >= Wq ? 1 : 0, xw = i - side * Wq;
        const int b = xw * CORE, w0 = b >> 6, sh = b & 63;
        u64 v = bits[side][w0] >> sh;
        if (sh) v |= bits[side][w0 + 1] << (64 - sh);
        v &= (1ull << CORE) - 1;
        const size_t o = (((size_t)n * 2 + side) * H + y) * Wq + xw;
        plane_o[o] = v;
        if (plane_x) plane_x[o] = v;
    }
}

// the window of row r (a row of a plane, Wq words) around word xw
template <int CORE, int HALO>
__device__ __forceinline__ u64 window(const u64* __restrict__ r, int xw, int Wq) {
    const u64 lw = xw > 0 ? r[xw - 1] : 0, rw = xw + 1 < Wq ? r[xw + 1] : 0;
    return (lw >> (CORE - HALO)) | (r[xw] << HALO) | (rw << (HALO + CORE));
}
// bit x of a row of plane words
template <int CORE>
__device__ __forceinline__ unsigned pixel(const u64* row, int x) {
    const int xw = x / CORE;
    return (unsigned)(row[xw] >> (x - xw * CORE)) & 1u;
}

// the neighbours of window c clockwise from north; u and d are the windows of the rows above and below. Bit i + 1 is the pixel to the
// east of bit i.
struct Ring {
    u64 p2, p3, p4, p5, p6, p7, p8, p9;
};
__device__ __forceinline__ Ring ring(u64 u, u64 c, u64 d) { return {u, u >> 1, c >> 1, d >> 1, d, d << 1, c << 1, u << 1}; }

// A thread's place in a step launch of grid N * nsides * ntiles * Wq (ntiles = ceil(H / (ROWS - 2 * HALO))), block ROWS. slot: n * 2 +
// side, the index of the image side's counter; y: the thread's row; in_image: y lies inside the image, and row is then the offset of
// that row's Wq words in a plane; core_row: the thread stores its core bits. skip (the same for the whole workgroup): the launch before
// counted nothing here, a fixed point that `out` already holds.
struct Tile {
    int n, slot, xw, y;
    size_t row;
    bool skip, in_image, core_row;
};
// also zeroes the rim rows of the two LDS row buffers and the workgroup's counts; prev: the counters of the launch before, or nullptr
template <int HALO, int ROWS, int NRED>
__device__ __forceinline__ Tile tile_open(u64 (&rows)[2][ROWS + 2], unsigned (&red)[NRED], const uint32_t* __restrict__ prev, int H, int Wq,
                                          int nsides, int ntiles) {
    Tile t;
    const int per = ntiles * Wq, z = blockIdx.x / per, rest = blockIdx.x - z * per;
    t.n = z / nsides;
    t.slot = t.n * 2 + (z - t.n * nsides);
    t.skip = prev && prev[t.slot] == 0;
    const int tid = threadIdx.x, ty = rest / Wq;
    t.xw = rest - ty * Wq;
    t.y = ty * (ROWS - 2 * HALO) - HALO + tid;
    t.in_image = t.y >= 0 && t.y < H;
    t.row = (size_t)t.slot * H * Wq + (size_t)t.y * Wq;
    if (tid == 0 && !t.skip) {
        rows[0][0] = rows[1][0] = rows[0][ROWS + 1] = rows[1][ROWS + 1] = 0;
#pragma unroll
        for (int k = 0; k < NRED; ++k) red[k] = 0;
    }
    t.core_row = tid >= HALO && tid < ROWS - HALO && t.y < H;
    return t;
}
// Core rows store the core bits of c. Their counts n0 (and n1) are summed in LDS and added to dst0[slot] (and, where given, dst1[slot])
// with one integer atomic per workgroup.
template <int CORE, int HALO, int NRED>
__device__ __forceinline__ void tile_close(const Tile& t, u64* __restrict__ out, u64 c, unsigned (&red)[NRED], unsigned n0,
                                           uint32_t* __restrict__ dst0, unsigned n1 = 0, uint32_t* __restrict__ dst1 = nullptr) {
    if (t.core_row) {
        out[t.row + t.xw] = (c >> HALO) & ((1ull << CORE) - 1);
        if (n0) atomicAdd(&red[0], n0);
        if (NRED > 1 && n1) atomicAdd(&red[NRED - 1], n1);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (red[0]) atomicAdd(&dst0[t.slot], red[0]);
        if (NRED > 1 && dst1 && red[NRED - 1]) atomicAdd(&dst1[t.slot], red[NRED - 1]);
    }
}

}  // namespace bitrows
