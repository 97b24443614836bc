// Road segments of a centre-line (include/rsu_segments.h): the junction pixels J (crossing number >= 3) of the predicted mask
// P = {counted and prob >= threshold} and of the truth mask T = {label == 1}, the node zones Z = A and dilate8(J), the segments
// S = A \ Z, both labelled by components.hip's cc_label, and one row of integers per segment: pixels, orthogonal and diagonal links,
// contacts with node zones, line ends and the two nodes it joins.
//
// ws: the float32 planes [4 N][H][W] (plane k * N + n: k = 0 S_P, 1 S_T, 2 Z_P, 3 Z_T of image n, 1.0 / 0.0), the labels int32 of the
// same shape, the labelling's parents and totals (cc_label's own workspace; after the flatten launch nothing reads the parents and the
// place launch keeps every root's rank at the root's position there), then the block counts [4 N][nblk], nblk = ceil(H W / SG_BLOCK).
//
//   k_seg_classify  one workgroup per SG_TW x SG_TH tile: A of the tile and a two-pixel halo into LDS (bit 0 = P, bit 1 = T), J of the
//                   tile and a one-pixel halo from it, then Z = A and any J in the 3 x 3, S = A and not Z. Writes the four planes.
//   (cc_label)      the tile, merge and flatten launches of components.hip on the 4 N planes at threshold 0.5, connectivity 8.
//   k_seg_count     the roots (label == index + 1) of every block of SG_BLOCK pixels of every plane: one ballot per wave.
//   k_seg_scan      one workgroup per image and side: the exclusive scan of its S plane's block counts in LDS (in place), the sum of
//                   its Z plane's; writes counts.
//   k_seg_place     every root of an S plane gets its rank: the block's offset, the waves before it, the lanes before it (ballot,
//                   popcount). The rank goes to the root's position in the parents; a rank below max_edges initialises its row:
//                   label, pixels, zeros and the sentinels of the two node ids.
//   k_seg_measure   one thread per pixel of the S planes. A segment pixel reads the labels of its 3 x 3 in both planes, counts its links
//                   towards E, SW, S and SE, the distinct zone labels around it and its end flag, and adds what is not zero to its
//                   segment's row: integer add / min / max atomics, all order-free. Writes seg_* and node_* where asked. (Runs of
//                   equal labels in adjacent lanes are NOT merged inside a wave first: the launch is a tenth of the call's kernel time,
//                   behind the labelling's tile and merge launches -- profiles/r26/segments.txt -- so the variant was not built.)
//   k_seg_finish    one workgroup per image and side: untouched sentinels become 0, the stored rows are classified and summed in LDS,
//                   one 64-bit integer atomic add per non-zero counter goes to acc.
// The only float operation is `p >= threshold`. No flag between workgroups, no grid-wide barrier, no float atomic.
#include "segments.h"

#include "components.h"

#define SG_BLOCK 256   // pixels per block of the compaction, threads of every launch
#define SG_TW 64       // the classify tile: SG_TW x SG_TH pixels, one per thread and row pass
#define SG_TH 16

namespace {

typedef unsigned long long u64;
constexpr int SG_HALO = 2;
constexpr int SG_LW = SG_TW + 2 * SG_HALO, SG_LH = SG_TH + 2 * SG_HALO;   // A in LDS
constexpr int SG_JW = SG_TW + 2, SG_JH = SG_TH + 2;                       // J in LDS
constexpr int SG_NONE_A = 0x7fffffff, SG_NONE_B = -0x7fffffff - 1;        // the sentinels of node_a (a minimum) and node_b (a maximum)
static_assert(SG_BLOCK == 256 && SG_BLOCK % 64 == 0, "four waves per block");
static_assert((long)SG_MAX_SIDE * SG_MAX_SIDE <= CC_MAX_PIXELS, "cc_label's area field holds a segment's pixel count");

// the eight neighbours clockwise from north: p2 = N, p3 = NE, p4 = E, p5 = SE, p6 = S, p7 = SW, p8 = W, p9 = NW
__device__ constexpr int SG_DY[8] = {-1, -1, 0, 1, 1, 1, 0, -1};
__device__ constexpr int SG_DX[8] = {0, 1, 1, 1, 0, -1, -1, -1};

// ring: bit i = p_{i + 2}. X = the number of i with p_i == 0 and p_{i + 1} == 1, cyclic
__device__ __forceinline__ int sg_crossings(unsigned ring) {
    const unsigned next = ((ring >> 1) | (ring << 7)) & 0xffu;
    return __popc(~ring & next);
}

// grid N * tiles_y * tiles_x. LAB: labels given (else every pixel counted, T empty)
template <bool LAB>
__global__ void __launch_bounds__(SG_BLOCK) k_seg_classify(const float* __restrict__ prob, float threshold, const int64_t* __restrict__ labels,
                                                           float* __restrict__ planes, int N, int H, int W, int tiles_x, int tiles_y) {
    __shared__ unsigned char a[SG_LH][SG_LW];
    __shared__ unsigned char j[SG_JH][SG_JW];
    const int tid = threadIdx.x;
    const unsigned per = (unsigned)tiles_x * (unsigned)tiles_y;
    const unsigned n = blockIdx.x / per, t = blockIdx.x % per;
    const int y0 = (int)(t / (unsigned)tiles_x) * SG_TH, x0 = (int)(t % (unsigned)tiles_x) * SG_TW;
    const size_t HW = (size_t)H * W, img = (size_t)n * HW;
    for (int i = tid; i < SG_LH * SG_LW; i += SG_BLOCK) {
        const int ly = i / SG_LW, lx = i - ly * SG_LW, y = y0 - SG_HALO + ly, x = x0 - SG_HALO + lx;
        unsigned v = 0;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const size_t g = img + (size_t)y * W + x;
            const int64_t l = LAB ? labels[g] : 0;
            const bool counted = l == 0 || l == 1;
            v = (counted && prob[g] >= threshold ? 1u : 0u) | (LAB && l == 1 ? 2u : 0u);   // (NaN compares false)
        }
        a[ly][lx] = (unsigned char)v;
    }
    __syncthreads();
    for (int i = tid; i < SG_JH * SG_JW; i += SG_BLOCK) {
        const int jy = i / SG_JW, jx = i - jy * SG_JW, ly = jy + 1, lx = jx + 1;   // (the same pixel in a)
        const unsigned c = a[ly][lx];
        unsigned ring0 = 0, ring1 = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const unsigned v = a[ly + SG_DY[k]][lx + SG_DX[k]];
            ring0 |= (v & 1u) << k;
            ring1 |= ((v >> 1) & 1u) << k;
        }
        j[jy][jx] = (unsigned char)(((c & 1u) && sg_crossings(ring0) >= 3 ? 1u : 0u) | ((c & 2u) && sg_crossings(ring1) >= 3 ? 2u : 0u));
    }
    __syncthreads();
    const size_t plane = (size_t)N * HW;
    for (int i = tid; i < SG_TH * SG_TW; i += SG_BLOCK) {
        const int ty = i / SG_TW, tx = i - ty * SG_TW, y = y0 + ty, x = x0 + tx;
        if (y >= H || x >= W) continue;
        unsigned near = 0;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy)
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) near |= j[ty + dy][tx + dx];
        const unsigned c = a[ty + SG_HALO][tx + SG_HALO], z = c & near, s = c & ~near;
        const size_t g = img + (size_t)y * W + x;
        planes[g] = (s & 1u) ? 1.0f : 0.0f;
        planes[plane + g] = (s & 2u) ? 1.0f : 0.0f;
        planes[2 * plane + g] = (z & 1u) ? 1.0f : 0.0f;
        planes[3 * plane + g] = (z & 2u) ? 1.0f : 0.0f;
    }
}

// a block's root count from the flags of its four waves; every thread gets it. `before`: the roots in the waves before this one
__device__ __forceinline__ int sg_block_roots(bool root, int* wsum, int& before, u64& ballot) {
    const int tid = threadIdx.x, wave = tid >> 6;
    ballot = __ballot(root);
    if ((tid & 63) == 0) wsum[wave] = __popcll(ballot);
    __syncthreads();
    int total = 0;
    before = 0;
#pragma unroll
    for (int w = 0; w < SG_BLOCK / 64; ++w) {
        const int v = wsum[w];
        if (w < wave) before += v;
        total += v;
    }
    return total;
}

// grid 4 N * nblk
__global__ void __launch_bounds__(SG_BLOCK) k_seg_count(const int* __restrict__ lab, int* __restrict__ bc, unsigned HW, unsigned nblk) {
    __shared__ int wsum[SG_BLOCK / 64];
    const unsigned q = blockIdx.x / nblk, b = blockIdx.x % nblk, i = b * SG_BLOCK + threadIdx.x;
    const bool root = i < HW && (unsigned)lab[(size_t)q * HW + i] == i + 1;
    int before;
    u64 ballot;
    const int total = sg_block_roots(root, wsum, before, ballot);
    if (threadIdx.x == 0) bc[blockIdx.x] = total;
}

// grid 2 N (plane q = side * N + n), block SG_BLOCK. bc [4 N][nblk]: the S planes' counts become exclusive offsets
__global__ void __launch_bounds__(SG_BLOCK) k_seg_scan(int* __restrict__ bc, int32_t* __restrict__ counts, unsigned N, unsigned nblk) {
    __shared__ int part[SG_BLOCK];
    __shared__ int nodes;
    const int tid = threadIdx.x;
    const unsigned q = blockIdx.x, side = q / N, n = q % N;
    int* s = bc + (size_t)q * nblk;
    const int* z = bc + (size_t)(q + 2 * N) * nblk;
    const unsigned chunk = (nblk + SG_BLOCK - 1) / SG_BLOCK, lo = tid * chunk, hi = lo + chunk < nblk ? lo + chunk : nblk;
    if (tid == 0) nodes = 0;
    int mine = 0, zs = 0;
    for (unsigned i = lo; i < hi; ++i) mine += s[i];
    for (unsigned i = tid; i < nblk; i += SG_BLOCK) zs += z[i];
    part[tid] = mine;
    __syncthreads();
    if (zs) atomicAdd(&nodes, zs);
    for (int d = 1; d < SG_BLOCK; d <<= 1) {   // an inclusive scan of the 256 partial sums
        const int v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = part[tid] - mine;
    for (unsigned i = lo; i < hi; ++i) {
        const int c = s[i];
        s[i] = run;
        run += c;
    }
    if (tid == 0) {
        counts[(size_t)n * 4 + 2 * side] = part[SG_BLOCK - 1];
        counts[(size_t)n * 4 + 2 * side + 1] = nodes;
    }
}

// grid 2 N * nblk. rank: the S planes' part of the labelling's parents. edges0 / edges1: [N][max_edges][8]
__global__ void __launch_bounds__(SG_BLOCK) k_seg_place(const int* __restrict__ lab, const int* __restrict__ tot, const int* __restrict__ bc,
                                                        int* __restrict__ rank, int32_t* __restrict__ edges0, int32_t* __restrict__ edges1,
                                                        int max_edges, unsigned N, unsigned HW, unsigned nblk) {
    __shared__ int wsum[SG_BLOCK / 64];
    const unsigned q = blockIdx.x / nblk, b = blockIdx.x % nblk, i = b * SG_BLOCK + threadIdx.x;
    const size_t g = (size_t)q * HW + i;
    const bool root = i < HW && (unsigned)lab[g] == i + 1;
    int before;
    u64 ballot;
    sg_block_roots(root, wsum, before, ballot);
    if (!root) return;
    const int r = bc[blockIdx.x] + before + __popcll(ballot & ((1ull << (threadIdx.x & 63)) - 1ull));
    rank[g] = r;
    int32_t* edges = q / N ? edges1 : edges0;
    if (r >= max_edges || !edges) return;
    int32_t* row = edges + ((size_t)(q % N) * max_edges + r) * 8;
    row[0] = (int)(i + 1);
    row[1] = tot[g] & CC_AREA;
    row[2] = row[3] = row[6] = row[7] = 0;
    row[4] = SG_NONE_A;
    row[5] = SG_NONE_B;
}

// grid 2 N * nblk. lab: [4 N][HW], the S planes then the Z planes
__global__ void __launch_bounds__(SG_BLOCK) k_seg_measure(const int* __restrict__ lab, const int* __restrict__ rank, int32_t* __restrict__ edges0,
                                                          int32_t* __restrict__ edges1, int32_t* __restrict__ seg0, int32_t* __restrict__ seg1,
                                                          int32_t* __restrict__ node0, int32_t* __restrict__ node1, int max_edges, unsigned N,
                                                          int H, int W, unsigned nblk) {
    const unsigned HW = (unsigned)(H * W);
    const unsigned q = blockIdx.x / nblk, b = blockIdx.x % nblk, i = b * SG_BLOCK + threadIdx.x;
    if (i >= HW) return;
    const unsigned side = q / N, n = q % N;
    const int* ls = lab + (size_t)q * HW;
    const int* lz = lab + (size_t)(q + 2 * N) * HW;
    int32_t* seg = side ? seg1 : seg0;
    int32_t* node = side ? node1 : node0;
    const size_t o = (size_t)n * HW + i;
    const int label = ls[i];
    if (!label) {
        if (seg) seg[o] = 0;
        if (node) node[o] = lz[i];
        return;
    }
    const int y = (int)(i / (unsigned)W), x = (int)(i - (unsigned)y * (unsigned)W);
    int s[8], z[8];   // the segment and the zone labels of the eight neighbours (indices are compile-time constants: registers)
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const int yy = y + SG_DY[k], xx = x + SG_DX[k];
        const bool in = yy >= 0 && yy < H && xx >= 0 && xx < W;
        const int at = in ? yy * W + xx : 0;
        s[k] = in ? ls[at] : 0;
        z[k] = in ? lz[at] : 0;
    }
    unsigned ring = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) ring |= (s[k] | z[k]) ? 1u << k : 0u;
    const bool end = sg_crossings(ring) <= 1 && __popc(ring) <= 3;
    // links towards E (2), SE (3), S (4), SW (5); a diagonal one counts only if neither pixel 4-adjacent to both is in A
    int ortho = (s[2] ? 1 : 0) + (s[4] ? 1 : 0);
    int diag = (s[3] && !(ring & 0x14u) ? 1 : 0) + (s[5] && !(ring & 0x50u) ? 1 : 0);
    // contacts: the distinct zone labels around the pixel; orthogonal if the label is among N, E, S, W
    int contacts = 0, lo = SG_NONE_A, hi = SG_NONE_B;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        bool first = z[k] != 0;
#pragma unroll
        for (int m = 0; m < k; ++m) first = first && z[m] != z[k];
        if (!first) continue;
        const bool edge = z[0] == z[k] || z[2] == z[k] || z[4] == z[k] || z[6] == z[k];
        ++contacts;
        ortho += edge ? 1 : 0;
        diag += edge ? 0 : 1;
        lo = min(lo, z[k]);
        hi = max(hi, z[k]);
    }
    const int id = -(int)(i + 1);
    if (end) {
        lo = min(lo, id);
        hi = max(hi, id);
    }
    if (seg) seg[o] = label;
    if (node) node[o] = end ? id : 0;
    const int r = rank[(size_t)q * HW + (unsigned)(label - 1)];
    int32_t* edges = side ? edges1 : edges0;
    if (r >= max_edges || !edges) return;
    int32_t* row = edges + ((size_t)n * max_edges + r) * 8;
    if (ortho) atomicAdd(&row[2], ortho);
    if (diag) atomicAdd(&row[3], diag);
    if (lo != SG_NONE_A) {
        atomicMin(&row[4], lo);
        atomicMax(&row[5], hi);
    }
    if (contacts) atomicAdd(&row[6], contacts);
    if (end) atomicAdd(&row[7], 1);
}

// grid 2 N, block SG_BLOCK
__global__ void __launch_bounds__(SG_BLOCK) k_seg_finish(int32_t* __restrict__ edges0, int32_t* __restrict__ edges1,
                                                         const int32_t* __restrict__ counts, u64* __restrict__ acc, int max_edges, unsigned N) {
    __shared__ u64 sums[8];
    const int tid = threadIdx.x;
    const unsigned q = blockIdx.x, side = q / N, n = q % N;
    int32_t* edges = side ? edges1 : edges0;
    const int count = counts[(size_t)n * 4 + 2 * side], stored = count < max_edges ? count : max_edges;
    if (!edges || !stored) return;   // (the same for the whole workgroup)
    if (tid < 8) sums[tid] = 0;
    __syncthreads();
    u64 v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (int r = tid; r < stored; r += SG_BLOCK) {
        int32_t* row = edges + ((size_t)n * max_edges + r) * 8;
        if (row[4] == SG_NONE_A) row[4] = row[5] = 0;
        const int touch = row[6] + row[7];
        v[0] += 1;
        v[1] += (u64)row[1];
        v[2] += (u64)row[2];
        v[3] += (u64)row[3];
        v[4] += row[6] == 1 && row[7] == 1;
        v[5] += row[6] == 0 && row[7] >= 1;
        v[6] += touch == 0;
        v[7] += touch > 2;
    }
#pragma unroll
    for (int k = 0; k < 8; ++k) {   // summed inside the wave first: 256 LDS atomics on one address would go one by one
        u64 x = v[k];
#pragma unroll
        for (int d = 32; d; d >>= 1) x += __shfl_xor(x, d);
        if ((tid & 63) == 0 && x) atomicAdd(&sums[k], x);
    }
    __syncthreads();
    if (acc && tid < 8 && sums[tid]) atomicAdd(&acc[side * 8 + tid], sums[tid]);
}

inline unsigned sg_nblk(int H, int W) { return ((unsigned)(H * W) + SG_BLOCK - 1) / SG_BLOCK; }

}  // namespace

size_t sg_ws_bytes(int N, int H, int W) {
    const size_t total = (size_t)4 * N * H * W;
    return (total * 16 + (size_t)4 * N * sg_nblk(H, W) * sizeof(int) + 7) / 8 * 8;
}

int sg_launches(int H, int W) { return 8 + cc_levels(H, W); }

hipError_t sg_line_segments(const float* prob, float threshold, const int64_t* labels, int max_edges, int32_t* edges_pred, int32_t* edges_true,
                            int32_t* counts, int32_t* seg_pred, int32_t* seg_true, int32_t* node_pred, int32_t* node_true,
                            unsigned long long* acc, void* ws, int N, int H, int W, hipStream_t st) {
    const size_t total = (size_t)4 * N * H * W;
    const unsigned HW = (unsigned)(H * W), nblk = sg_nblk(H, W);
    float* planes = (float*)ws;
    int* lab = (int*)(planes + total);
    int* par = lab + total;   // cc_label's workspace: the parents, then the totals
    int* tot = par + total;
    int* bc = tot + total;
    const int tx = (W + SG_TW - 1) / SG_TW, ty = (H + SG_TH - 1) / SG_TH;
    const dim3 cgrid((unsigned)((size_t)N * tx * ty)), block(SG_BLOCK);
    if (labels)
        hipLaunchKernelGGL(k_seg_classify<true>, cgrid, block, 0, st, prob, threshold, labels, planes, N, H, W, tx, ty);
    else
        hipLaunchKernelGGL(k_seg_classify<false>, cgrid, block, 0, st, prob, threshold, labels, planes, N, H, W, tx, ty);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    e = cc_label(planes, 0.5f, 8, 0, lab, nullptr, nullptr, par, 4 * N, H, W, st);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_seg_count, dim3(4u * (unsigned)N * nblk), block, 0, st, (const int*)lab, bc, HW, nblk);
    hipLaunchKernelGGL(k_seg_scan, dim3(2u * (unsigned)N), block, 0, st, bc, counts, (unsigned)N, nblk);
    hipLaunchKernelGGL(k_seg_place, dim3(2u * (unsigned)N * nblk), block, 0, st, (const int*)lab, (const int*)tot, (const int*)bc, par, edges_pred,
                       edges_true, max_edges, (unsigned)N, HW, nblk);
    hipLaunchKernelGGL(k_seg_measure, dim3(2u * (unsigned)N * nblk), block, 0, st, (const int*)lab, (const int*)par, edges_pred, edges_true, seg_pred,
                       seg_true, node_pred, node_true, max_edges, (unsigned)N, H, W, nblk);
    hipLaunchKernelGGL(k_seg_finish, dim3(2u * (unsigned)N), block, 0, st, edges_pred, edges_true, (const int32_t*)counts, (u64*)acc, max_edges,
                       (unsigned)N);
    return hipGetLastError();
}
