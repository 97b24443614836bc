// Ordered polylines of road segments (include/rsu_paths.h): the pixels of every stored segment of one side of rsu_line_segments, ranked
// along the segment by pointer jumping over arcs. Integer only; every result is a function of the inputs alone.
//
// Path links: two pixels of S = {seg != 0} are linked iff they are 4-adjacent, or diagonal neighbours with neither common 4-neighbour in
// S. The eight directions are numbered in ascending row-major offset (NW, N, NE, W, E, SW, S, SE: the opposite of d is 7 - d), so a
// pixel's link mask lists its neighbours in ascending index and `slot` s is its s-th set bit. An ARC is (pixel, slot), number
// 2 * (n H W + index) + slot, and stands for the step from the pixel to that neighbour. Its 64-bit word holds the arc reached in the low
// half and the hops made in the high half. A FINAL arc (its head is a STOP pixel: a terminal of an open segment, the smallest pixel of a
// ring; or a dead end) holds itself and 0 hops, with PT_GOOD set where it enters the segment's start pixel (for a ring: and leaves from
// the start's smaller neighbour). The flag travels with the arc number through the doublings.
//
// ws: arcs A and B, u64 [N][H][W][2] each; the pixel plane int32 [N][H][W]: row << 8 | link mask at the pixels of a stored row, -1
// elsewhere; minterm and branch, int32 [N][max_edges] each; the changed-arc counts int32 [max(R, 1)][N].
//
//   k_paths_init     minterm = PT_NONE, branch = 0, counts = 0.
//   k_paths_classify one workgroup per PT_TW x PT_TH tile: the labels of the tile and a one-pixel halo into LDS, every pixel's link mask
//                    from it, the label's row by binary search over the ascending labels of the stored rows; integer min / or atomics
//                    give every row its smallest terminal (link degree <= 1) and its branched flag (a degree >= 3). Writes the plane.
//   k_paths_rows     one workgroup per image: the kind of every stored row, the exclusive scan of the ordered rows' pixel counts in LDS,
//                    info.
//   k_paths_arcs     one thread per pixel: the two arcs of every pixel of a stored row into A.
//   k_paths_jump     R launches, one doubling each, A -> B, B -> A, ...: no workgroup reads what another wrote in the same launch. A
//                    launch adds its changed arcs to its own count of the image (one integer atomic per workgroup of PT_JUMP x 256
//                    pixels); the next launch returns at once for an image whose count stayed 0 (both buffers then hold the same
//                    words).
//   k_paths_emit     one thread per pixel: position 0 at the start pixel, hops + 1 of the arc whose final arc carries PT_GOOD elsewhere;
//                    writes paths (below max_points) and pos.
// No float operation, no flag between workgroups, no grid-wide barrier.
#include "paths.h"

#define PT_BLOCK 256   // threads of every launch
#define PT_TW 64       // the classify tile: PT_TW x PT_TH pixels
#define PT_TH 16
#define PT_JUMP 8      // pixels per thread of a jump launch

namespace {

typedef unsigned long long u64;
constexpr unsigned PT_GOOD = 0x80000000u, PT_ARC = 0x7fffffffu;
constexpr int PT_NONE = 0x7fffffff;
constexpr int PT_LW = PT_TW + 2, PT_LH = PT_TH + 2;
static_assert(PT_BLOCK == 256 && (PT_TW * PT_TH) % PT_BLOCK == 0, "whole passes over the tile");
static_assert(PT_MAX_EDGES <= (1 << 16), "a row index and the link mask share 24 bits of the pixel plane");

// ascending row-major offset: NW, N, NE, W, E, SW, S, SE
__device__ constexpr int PT_DY[8] = {-1, -1, -1, 0, 0, 1, 1, 1};
__device__ constexpr int PT_DX[8] = {-1, 0, 1, -1, 1, -1, 0, 1};

// the row-major offset of direction d (a run-time d: no table in memory); dx + 1 of the eight directions, two bits each: 0x9224
__device__ __forceinline__ int pt_offset(int d, int W) {
    const int dy = d < 3 ? -1 : (d < 5 ? 0 : 1), dx = (int)((0x9224u >> (2 * d)) & 3u) - 1;
    return dy * W + dx;
}
__device__ __forceinline__ u64 pt_word(unsigned arc, unsigned hops) { return (u64)arc | ((u64)hops << 32); }
__device__ __forceinline__ int pt_stored(const int32_t* counts, unsigned n, int side, int max_edges) {
    const int c = counts[(size_t)n * 4 + 2 * side];
    return c < 0 ? 0 : (c < max_edges ? c : max_edges);
}

// grid-stride over minterm, branch (rows each) and the counts (ncnt)
__global__ void __launch_bounds__(PT_BLOCK) k_paths_init(int* __restrict__ minterm, int* __restrict__ branch, int* __restrict__ cnt, size_t rows,
                                                         size_t ncnt) {
    const size_t step = (size_t)gridDim.x * PT_BLOCK;
    for (size_t i = (size_t)blockIdx.x * PT_BLOCK + threadIdx.x; i < rows; i += step) {
        minterm[i] = PT_NONE;
        branch[i] = 0;
    }
    for (size_t i = (size_t)blockIdx.x * PT_BLOCK + threadIdx.x; i < ncnt; i += step) cnt[i] = 0;
}

// grid N * tiles_y * tiles_x
__global__ void __launch_bounds__(PT_BLOCK) k_paths_classify(const int32_t* __restrict__ seg, const int32_t* __restrict__ edges,
                                                             const int32_t* __restrict__ counts, int side, int max_edges, int* __restrict__ plane,
                                                             int* __restrict__ minterm, int* __restrict__ branch, int H, int W, int tiles_x,
                                                             int tiles_y) {
    __shared__ int lab[PT_LH][PT_LW];
    const int tid = threadIdx.x;
    const unsigned per = (unsigned)tiles_x * (unsigned)tiles_y;
    const unsigned n = blockIdx.x / per, t = blockIdx.x % per;
    const int y0 = (int)(t / (unsigned)tiles_x) * PT_TH, x0 = (int)(t % (unsigned)tiles_x) * PT_TW;
    const size_t HW = (size_t)H * W, img = (size_t)n * HW;
    for (int i = tid; i < PT_LH * PT_LW; i += PT_BLOCK) {
        const int ly = i / PT_LW, lx = i - ly * PT_LW, y = y0 - 1 + ly, x = x0 - 1 + lx;
        lab[ly][lx] = y >= 0 && y < H && x >= 0 && x < W ? seg[img + (size_t)y * W + x] : 0;   // (outside an image: background)
    }
    __syncthreads();
    const int stored = pt_stored(counts, n, side, max_edges);
    const int32_t* rows = edges + (size_t)n * max_edges * 8;
    for (int i = tid; i < PT_TH * PT_TW; i += PT_BLOCK) {
        const int ty = i / PT_TW, tx = i - ty * PT_TW, y = y0 + ty, x = x0 + tx;
        if (y >= H || x >= W) continue;
        const int label = lab[ty + 1][tx + 1];
        int out = -1;
        if (label) {
            unsigned s = 0;   // bit d: the neighbour in direction d is in S
#pragma unroll
            for (int d = 0; d < 8; ++d) s |= lab[ty + 1 + PT_DY[d]][tx + 1 + PT_DX[d]] ? 1u << d : 0u;
            // a diagonal link only where neither pixel 4-adjacent to both is in S: NW (N, W), NE (N, E), SW (W, S), SE (E, S)
            unsigned mask = s & 0x5au;
            mask |= (s & 0x01u) && !(s & 0x0au) ? 0x01u : 0u;
            mask |= (s & 0x04u) && !(s & 0x12u) ? 0x04u : 0u;
            mask |= (s & 0x20u) && !(s & 0x48u) ? 0x20u : 0u;
            mask |= (s & 0x80u) && !(s & 0x50u) ? 0x80u : 0u;
            int lo = 0, hi = stored;   // the first stored row whose label is not below this one
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (rows[(size_t)mid * 8] < label)
                    lo = mid + 1;
                else
                    hi = mid;
            }
            if (lo < stored && rows[(size_t)lo * 8] == label) {
                out = (lo << 8) | (int)mask;
                const int deg = __popc(mask);
                const size_t r = (size_t)n * max_edges + lo;
                if (deg >= 3) atomicOr(&branch[r], 1);
                if (deg <= 1) atomicMin(&minterm[r], y * W + x);
            }
        }
        plane[img + (size_t)y * W + x] = out;
    }
}

// grid N, block PT_BLOCK
__global__ void __launch_bounds__(PT_BLOCK) k_paths_rows(const int32_t* __restrict__ edges, const int32_t* __restrict__ counts, int side,
                                                         int max_edges, int max_len, const int* __restrict__ minterm,
                                                         const int* __restrict__ branch, int32_t* __restrict__ kind, int32_t* __restrict__ offsets,
                                                         int32_t* __restrict__ info) {
    __shared__ unsigned part[PT_BLOCK];
    __shared__ int kinds[3];
    const int tid = threadIdx.x;
    const unsigned n = blockIdx.x;
    const int stored = pt_stored(counts, n, side, max_edges);
    const int32_t* rows = edges + (size_t)n * max_edges * 8;
    const size_t base = (size_t)n * max_edges;
    const int chunk = (stored + PT_BLOCK - 1) / PT_BLOCK, lo = tid * chunk, hi = lo + chunk < stored ? lo + chunk : stored;
    if (tid < 3) kinds[tid] = 0;
    unsigned mine = 0;
    int c0 = 0, c1 = 0, c2 = 0;
    for (int r = lo; r < hi; ++r) {
        const int pixels = rows[(size_t)r * 8 + 1];
        const int k = pixels > max_len ? 3 : (branch[base + r] ? 2 : (minterm[base + r] != PT_NONE ? 0 : 1));
        kind[base + r] = k;
        mine += k <= 1 ? (unsigned)pixels : 0u;
        c0 += k == 0;
        c1 += k == 1;
        c2 += k >= 2;
    }
    part[tid] = mine;
    __syncthreads();
    if (c0) atomicAdd(&kinds[0], c0);
    if (c1) atomicAdd(&kinds[1], c1);
    if (c2) atomicAdd(&kinds[2], c2);
    for (int d = 1; d < PT_BLOCK; d <<= 1) {   // an inclusive scan of the 256 partial sums
        const unsigned v = tid >= d ? part[tid - d] : 0u;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    unsigned run = part[tid] - mine;
    int32_t* off = offsets + (size_t)n * ((size_t)max_edges + 1);
    for (int r = lo; r < hi; ++r) {
        const int pixels = rows[(size_t)r * 8 + 1];
        const int k = pixels > max_len ? 3 : (branch[base + r] ? 2 : (minterm[base + r] != PT_NONE ? 0 : 1));
        off[r] = (int)run;
        run += k <= 1 ? (unsigned)pixels : 0u;
    }
    if (tid == 0) {
        off[stored] = (int)part[PT_BLOCK - 1];
        info[(size_t)n * 4] = (int)part[PT_BLOCK - 1];
        info[(size_t)n * 4 + 1] = kinds[0];
        info[(size_t)n * 4 + 2] = kinds[1];
        info[(size_t)n * 4 + 3] = kinds[2];
    }
}

// the start pixel of an ordered row: its smallest terminal (open), label - 1 (ring)
__device__ __forceinline__ int pt_start(int k, const int32_t* rows, const int* minterm, size_t base, int row) {
    return k == 0 ? minterm[base + row] : rows[(size_t)row * 8] - 1;
}

// grid N * nblk
__global__ void __launch_bounds__(PT_BLOCK) k_paths_arcs(const int* __restrict__ plane, const int32_t* __restrict__ edges,
                                                         const int32_t* __restrict__ kind, const int* __restrict__ minterm, int max_edges,
                                                         u64* __restrict__ arcs, int W, unsigned HW, unsigned nblk) {
    const unsigned n = blockIdx.x / nblk, i = (blockIdx.x % nblk) * PT_BLOCK + threadIdx.x;
    if (i >= HW) return;
    const size_t img = (size_t)n * HW;
    const int inf = plane[img + i];
    if (inf < 0) return;
    const int row = inf >> 8;
    const size_t base = (size_t)n * max_edges;
    const int32_t* rows = edges + base * 8;
    const int k = kind[base + row];
    const unsigned a0 = 2u * (unsigned)(img + i);
    u64 word[2] = {pt_word(a0, 0), pt_word(a0 + 1, 0)};   // a slot without a neighbour, a row that is not ordered: a dead end
    if (k <= 1) {
        const int start = pt_start(k, rows, minterm, base, row);
        unsigned m = (unsigned)inf & 0xffu;
#pragma unroll
        for (int slot = 0; slot < 2; ++slot) {
            if (!m) break;
            const int d = __ffs(m) - 1, back = 7 - d;
            m &= m - 1;
            const unsigned wi = (unsigned)((int)i + pt_offset(d, W));   // (a set bit: that neighbour is inside the image)
            const int winf = plane[img + wi];
            if (winf < 0 || (winf >> 8) != row) continue;   // (inconsistent inputs only)
            const unsigned wmask = (unsigned)winf & 0xffu;
            const int wdeg = __popc(wmask);
            const bool stop = k == 0 ? wdeg <= 1 : (int)wi == start;
            if (stop) {
                const bool good = (int)wi == start && (k == 0 || __ffs(wmask) - 1 == back);
                word[slot] = pt_word((a0 + slot) | (good ? PT_GOOD : 0u), 0);
                continue;
            }
            const unsigned other = wmask & ~(1u << back);
            if (wdeg != 2 || !other) continue;
            const int od = __ffs(other) - 1;
            word[slot] = pt_word(2u * (unsigned)(img + wi) + (unsigned)__popc(wmask & ((1u << od) - 1u)), 1);
        }
    }
    arcs[a0] = word[0];
    arcs[a0 + 1] = word[1];
}

// grid N * jblk, jblk = ceil(H W / (PT_BLOCK * PT_JUMP)): PT_JUMP pixels per thread, PT_BLOCK apart. prev: the changed arcs of the launch
// before, per image (nullptr in the first); cur: this launch's. (One pixel per thread made 2 N H W / 512 workgroups add to one address
// per image: those atomics, one behind the other, were three quarters of the launch -- profiles/r30/paths.txt.)
__global__ void __launch_bounds__(PT_BLOCK) k_paths_jump(const u64* __restrict__ A, u64* __restrict__ B, const int* __restrict__ plane,
                                                         const int* __restrict__ prev, int* __restrict__ cur, unsigned HW, unsigned jblk) {
    __shared__ int moved;
    const unsigned n = blockIdx.x / jblk, i0 = (blockIdx.x % jblk) * (PT_BLOCK * PT_JUMP) + threadIdx.x;
    if (prev && prev[n] == 0) return;   // (the same for the whole workgroup)
    if (threadIdx.x == 0) moved = 0;
    __syncthreads();
    const size_t img = (size_t)n * HW;
    int inf[PT_JUMP];
#pragma unroll
    for (int k = 0; k < PT_JUMP; ++k) {
        const unsigned i = i0 + (unsigned)k * PT_BLOCK;
        inf[k] = i < HW ? plane[img + i] : -1;
    }
    int changed = 0;
#pragma unroll
    for (int k = 0; k < PT_JUMP; ++k) {
        if (inf[k] < 0) continue;
        const unsigned a0 = 2u * (unsigned)(img + i0 + (unsigned)k * PT_BLOCK);
#pragma unroll
        for (unsigned s = 0; s < 2; ++s) {
            const u64 old = A[a0 + s];
            const unsigned t = (unsigned)old & PT_ARC;
            u64 nw = old;
            if (t != a0 + s) {
                const u64 jb = A[t];
                nw = pt_word((unsigned)jb, (unsigned)(old >> 32) + (unsigned)(jb >> 32));
            }
            B[a0 + s] = nw;
            changed += nw != old;
        }
    }
    if (changed) atomicAdd(&moved, changed);
    __syncthreads();
    if (threadIdx.x == 0 && moved) atomicAdd(&cur[n], moved);
}

// grid N * nblk
__global__ void __launch_bounds__(PT_BLOCK) k_paths_emit(const u64* __restrict__ arcs, const int* __restrict__ plane, const int32_t* __restrict__ edges,
                                                         const int32_t* __restrict__ kind, const int32_t* __restrict__ offsets,
                                                         const int* __restrict__ minterm, int max_edges, int max_points, int32_t* __restrict__ paths,
                                                         int32_t* __restrict__ pos, unsigned HW, unsigned nblk) {
    const unsigned n = blockIdx.x / nblk, i = (blockIdx.x % nblk) * PT_BLOCK + threadIdx.x;
    if (i >= HW) return;
    const size_t g = (size_t)n * HW + i;
    const int inf = plane[g];
    int p = -1;
    if (inf >= 0) {
        const int row = inf >> 8;
        const size_t base = (size_t)n * max_edges;
        const int k = kind[base + row];
        if (k <= 1) {
            if ((int)i == pt_start(k, edges + base * 8, minterm, base, row)) {
                p = 0;
            } else {
                const unsigned a0 = 2u * (unsigned)g;
#pragma unroll
                for (unsigned s = 0; s < 2; ++s) {
                    const u64 w = arcs[a0 + s];
                    if ((unsigned)w & PT_GOOD) p = (int)(unsigned)(w >> 32) + 1;
                }
            }
            if (p >= 0) {
                const long at = (long)offsets[(size_t)n * ((size_t)max_edges + 1) + row] + p;
                if (at >= 0 && at < max_points) paths[(size_t)n * max_points + at] = (int)i;
            }
        }
    }
    if (pos) pos[g] = p + 1;
}

inline unsigned pt_nblk(int H, int W) { return ((unsigned)(H * W) + PT_BLOCK - 1) / PT_BLOCK; }

}  // namespace

int pt_rounds(int max_len) {
    int r = 0;
    while ((1L << r) < max_len) ++r;
    return r;
}

size_t pt_ws_bytes(int N, int H, int W, int max_edges, int max_len) {
    const size_t px = (size_t)N * H * W;
    const int R = pt_rounds(max_len);
    return (px * 36 + ((size_t)2 * N * max_edges + (size_t)(R > 1 ? R : 1) * N) * sizeof(int) + 7) / 8 * 8;
}

int pt_launches(int max_len) { return 5 + pt_rounds(max_len); }

hipError_t pt_segment_paths(const int32_t* seg, const int32_t* edges, const int32_t* counts, int side, int max_edges, int max_len, int max_points,
                            int32_t* paths, int32_t* offsets, int32_t* kind, int32_t* pos, int32_t* info, void* ws, int N, int H, int W,
                            hipStream_t st) {
    const size_t px = (size_t)N * H * W, rows = (size_t)N * max_edges;
    const unsigned HW = (unsigned)(H * W), nblk = pt_nblk(H, W);
    const int R = pt_rounds(max_len);
    u64* arcs[2] = {(u64*)ws, (u64*)ws + 2 * px};
    int* plane = (int*)(arcs[1] + 2 * px);
    int* minterm = plane + px;
    int* branch = minterm + rows;
    int* cnt = branch + rows;
    const size_t ncnt = (size_t)(R > 1 ? R : 1) * N;
    const dim3 block(PT_BLOCK), pixels((unsigned)N * nblk);
    hipLaunchKernelGGL(k_paths_init, dim3((unsigned)grid_for((long)(rows > ncnt ? rows : ncnt), PT_BLOCK, 1 << 16)), block, 0, st, minterm, branch, cnt,
                       rows, ncnt);
    const int tx = (W + PT_TW - 1) / PT_TW, ty = (H + PT_TH - 1) / PT_TH;
    hipLaunchKernelGGL(k_paths_classify, dim3((unsigned)((size_t)N * tx * ty)), block, 0, st, seg, edges, counts, side, max_edges, plane, minterm,
                       branch, H, W, tx, ty);
    hipLaunchKernelGGL(k_paths_rows, dim3((unsigned)N), block, 0, st, edges, counts, side, max_edges, max_len, (const int*)minterm, (const int*)branch,
                       kind, offsets, info);
    hipLaunchKernelGGL(k_paths_arcs, pixels, block, 0, st, (const int*)plane, edges, (const int32_t*)kind, (const int*)minterm, max_edges, arcs[0], W,
                       HW, nblk);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const unsigned jblk = (HW + PT_BLOCK * PT_JUMP - 1) / (PT_BLOCK * PT_JUMP);
    for (int r = 0; r < R; ++r)
        hipLaunchKernelGGL(k_paths_jump, dim3((unsigned)N * jblk), block, 0, st, (const u64*)arcs[r & 1], arcs[(r + 1) & 1], (const int*)plane,
                           r ? (const int*)(cnt + (size_t)(r - 1) * N) : (const int*)nullptr, cnt + (size_t)r * N, HW, jblk);
    hipLaunchKernelGGL(k_paths_emit, pixels, block, 0, st, (const u64*)arcs[R & 1], (const int*)plane, edges, (const int32_t*)kind,
                       (const int32_t*)offsets, (const int*)minterm, max_edges, max_points, paths, pos, HW, nblk);
    return hipGetLastError();
}
