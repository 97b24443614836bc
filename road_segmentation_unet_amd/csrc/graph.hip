// Centre-line pruning and node classification (include/rsu_graph.h): Gonzalez & Woods' morphological pruning of the predicted mask
// P = {counted and prob >= threshold} and of the truth mask T = {label == 1} -- L rounds that delete every END pixel, the END pixels of
// what is left, L rounds of a dilation of those inside the mask -- and the ends, isolated pixels and junction pixels of the result,
// evaluated bit-sliced on bit rows: the layout, the init launch and the step tile are those of bitrows.h, which thin.hip shares.
//
// ws holds bit planes in the layout of bitrows.h (CORE = GR_CORE). Plane O keeps the masks A; with L > 0 planes X0 and X1 are the working
// copies of the delete phase (step s reads X[s & 1] and writes the other) and planes E0 and E1 those of the regrow phase (launch g
// writes E[g & 1]). Behind them sit the counters, [D + G][N][2], D = ceil(L / GR_R) delete and G = ceil((L + 1) / GR_R) regrow launches.
//
//   k_graph_init    bitrows.h's init launch. Writes plane O (and X0); clears the counters.
//   k_graph_delete  bitrows.h's step tile: east and west are shifts of a thread's own window and north and south are its neighbours'
//                   registers, handed over through LDS (two buffers: one barrier per round). What is shifted in at the window's rim is
//                   wrong; the error walks one pixel per round and after GR_R of them has not left the halo. Deleted core pixels are
//                   counted per thread and added to the launch's own counter; the launch behind reads it and returns where it is 0:
//                   that image side was at its fixed point and both planes hold it.
//   k_graph_regrow  the same tile. A thread holds its window of E and the fixed window of A. The FIRST launch forms E = END(X1) from
//                   the delete phase's plane, which costs one pixel of halo, and carries GR_R - 1 rounds; the others carry GR_R. A
//                   launch counts the core pixels it added to E; where the count before it is 0 (for the first: the last delete
//                   launch's, a fixed point without END pixels) it returns and writes nothing.
//   k_graph_final   GR_FIN_ROWS rows per workgroup: B = X1 | E of rows y - 1 .. y + GR_FIN_ROWS into LDS (which E plane holds the result, if
//                   any, follows from the counters), one thread per word classifies its GR_CORE pixels, then every thread writes pixels.
//                   The eight counts go to acc through LDS integer atomics, one 64-bit atomic add per non-zero count per workgroup.
#include "graph.h"
#include "bitrows.h"

#ifndef GR_ROWS
#define GR_ROWS 128   // rows of a step tile, halo included: GR_ROWS - 2 * GR_HALO core rows
#endif

namespace {

namespace br = bitrows;
using br::u64;
constexpr int GR_INIT_THREADS = 256;
constexpr int GR_FIN_THREADS = 256, GR_FIN_ROWS = 4;
constexpr int GR_CROWS = GR_ROWS - 2 * GR_HALO;
constexpr u64 GR_COREBITS = (1ull << GR_CORE) - 1;
constexpr int GR_MAX_WQ = (GR_MAX_SIDE + GR_CORE - 1) / GR_CORE;
static_assert(GR_CROWS >= 1 && GR_ROWS % 64 == 0, "tile geometry");

// grid N * H, block GR_INIT_THREADS: bitrows.h init_row. plane_x: nullptr without a prune phase
template <bool LAB>
__global__ void __launch_bounds__(GR_INIT_THREADS) k_graph_init(const float* __restrict__ prob, float threshold,
                                                                const int64_t* __restrict__ labels, u64* __restrict__ plane_o,
                                                                u64* __restrict__ plane_x, uint32_t* __restrict__ counters, int nlaunch,
                                                                int N, int H, int W, int Wq) {
    br::init_row<LAB, GR_CORE, GR_INIT_THREADS, GR_MAX_SIDE>(prob, threshold, labels, plane_o, plane_x, counters, nlaunch, N, H, W, Wq);
}

// the sum of eight one-bit planes, bit-sliced: bit 0, bit 1 and "4 or more" of the count (full and half adders)
struct GrCount {
    u64 b0, b1, hi;
};
__device__ __forceinline__ GrCount gr_sum8(u64 a1, u64 a2, u64 a3, u64 a4, u64 a5, u64 a6, u64 a7, u64 a8) {
    const u64 x1 = a1 ^ a2, s1 = x1 ^ a3, c1 = (a1 & a2) | (x1 & a3);
    const u64 x2 = a4 ^ a5, s2 = x2 ^ a6, c2 = (a4 & a5) | (x2 & a6);
    const u64 s3 = a7 ^ a8, c3 = a7 & a8;
    const u64 x4 = s1 ^ s2, b0 = x4 ^ s3, c4 = (s1 & s2) | (x4 & s3);
    const u64 x5 = c1 ^ c2, s5 = x5 ^ c3, c5 = (c1 & c2) | (x5 & c3);
    return {b0, s5 ^ c4, c5 | (s5 & c4)};
}
// of the neighbours of window c (bitrows.h ring): n8, the number set; X, the number of 0 -> 1 steps around the cycle
struct GrNodes {
    GrCount n8, X;
};
__device__ __forceinline__ GrNodes gr_nodes(u64 u, u64 c, u64 d) {
    const auto [p2, p3, p4, p5, p6, p7, p8, p9] = br::ring(u, c, d);
    GrNodes r;
    r.n8 = gr_sum8(p2, p3, p4, p5, p6, p7, p8, p9);
    r.X = gr_sum8(~p2 & p3, ~p3 & p4, ~p4 & p5, ~p5 & p6, ~p6 & p7, ~p7 & p8, ~p8 & p9, ~p9 & p2);
    return r;
}
// END: a set pixel with X <= 1 and n8 <= 3
__device__ __forceinline__ u64 gr_end(u64 u, u64 c, u64 d) {
    const GrNodes k = gr_nodes(u, c, d);
    return c & ~(k.X.b1 | k.X.hi) & ~k.n8.hi;
}

// grid N * nsides * ntiles * Wq (ntiles = ceil(H / GR_CROWS)), block GR_ROWS. prev: the counters of the launch before (nullptr for the
// first step); cnt: this launch's. rounds in [1, GR_R].
__global__ void __launch_bounds__(GR_ROWS) k_graph_delete(const u64* __restrict__ in, u64* __restrict__ out, const uint32_t* __restrict__ prev,
                                                          uint32_t* __restrict__ cnt, int H, int Wq, int rounds, int nsides, int ntiles) {
    __shared__ u64 rows[2][GR_ROWS + 2];
    __shared__ unsigned red[1];
    const br::Tile t = br::tile_open<GR_HALO, GR_ROWS>(rows, red, prev, H, Wq, nsides, ntiles);
    if (t.skip) return;
    const int tid = threadIdx.x;
    u64 c = t.in_image ? br::window<GR_CORE, GR_HALO>(in + t.row, t.xw, Wq) : 0;
    const u64 core = GR_COREBITS << GR_HALO;
    unsigned total = 0;
    for (int it = 0; it < rounds; ++it) {
        u64* buf = rows[it & 1];
        buf[tid + 1] = c;
        __syncthreads();
        const u64 del = gr_end(buf[tid], c, buf[tid + 2]);
        c &= ~del;
        total += __popcll(del & core);
    }
    br::tile_close<GR_CORE, GR_HALO>(t, out, c, red, total, cnt);
}

// grid and block as k_graph_delete. FIRST: `in` is the delete phase's plane X1 and E starts as END(X1); else `in` is the E plane of the
// launch before. mask: plane O. rounds in [0, GR_R - 1] for the first launch, [1, GR_R] behind it.
template <bool FIRST>
__global__ void __launch_bounds__(GR_ROWS) k_graph_regrow(const u64* __restrict__ in, const u64* __restrict__ mask, u64* __restrict__ out,
                                                          const uint32_t* __restrict__ prev, uint32_t* __restrict__ cnt, int H, int Wq,
                                                          int rounds, int nsides, int ntiles) {
    __shared__ u64 rows[2][GR_ROWS + 2];
    __shared__ unsigned red[1];
    const br::Tile t = br::tile_open<GR_HALO, GR_ROWS>(rows, red, prev, H, Wq, nsides, ntiles);
    if (t.skip) return;   // nothing to grow, or E at its fixed point: see k_graph_final
    const int tid = threadIdx.x;
    u64 e = 0, a = 0;
    if (t.in_image) {
        e = br::window<GR_CORE, GR_HALO>(in + t.row, t.xw, Wq);
        a = br::window<GR_CORE, GR_HALO>(mask + t.row, t.xw, Wq);
    }
    const u64 core = GR_COREBITS << GR_HALO;
    unsigned before = 0;
    if (FIRST) {
        rows[1][tid + 1] = e;   // (buffer 1: the first round below takes buffer 0)
        __syncthreads();
        e = gr_end(rows[1][tid], e, rows[1][tid + 2]);
    } else {
        before = __popcll(e & core);
    }
    for (int it = 0; it < rounds; ++it) {
        u64* buf = rows[it & 1];
        buf[tid + 1] = e;
        __syncthreads();
        const u64 v = buf[tid] | e | buf[tid + 2];
        e = a & (v | (v << 1) | (v >> 1));
    }
    br::tile_close<GR_CORE, GR_HALO>(t, out, e, red, t.core_row ? __popcll(e & core) - before : 0u, cnt);
}

// grid N * nblk (nblk = ceil(H / GR_FIN_ROWS)), block GR_FIN_THREADS. x1: the plane behind the delete phase (plane O without one);
// e0, e1: the regrow planes; counters: [D + G][N][2] (nullptr without a prune phase)
template <bool LAB>
__global__ void __launch_bounds__(GR_FIN_THREADS) k_graph_final(const u64* __restrict__ x1, const u64* __restrict__ e0, const u64* __restrict__ e1,
                                                                const uint32_t* __restrict__ counters, int D, int G,
                                                                const int64_t* __restrict__ labels, float* __restrict__ out_pred,
                                                                int64_t* __restrict__ out_true, float* __restrict__ junc_pred,
                                                                int64_t* __restrict__ junc_true, u64* __restrict__ acc, int N, int H, int W,
                                                                int Wq, int nblk) {
    __shared__ u64 bw[2][GR_FIN_ROWS + 2][GR_MAX_WQ + 2];   // B of rows y0 - 1 .. y0 + GR_FIN_ROWS, a zero word to either side
    __shared__ u64 ow[2][2][GR_FIN_ROWS][GR_MAX_WQ];        // per side: B and the junction pixels of the rows written
    __shared__ unsigned sums[8];
    const int tid = threadIdx.x, n = blockIdx.x / nblk, y0 = (blockIdx.x - n * nblk) * GR_FIN_ROWS;
    constexpr int nsides = LAB ? 2 : 1;
    // the regrow plane that holds E, per side: launch g ran iff the count before it is not 0, and wrote E[g & 1]
    const u64* ep[2] = {nullptr, nullptr};
    if (counters) {
        for (int side = 0; side < nsides; ++side) {
            if (counters[((size_t)(D - 1) * N + n) * 2 + side] == 0) continue;   // the delete phase ended at a fixed point: no END pixel
            int g = 0;
            while (g + 1 < G && counters[((size_t)(D + g) * N + n) * 2 + side] != 0) ++g;
            ep[side] = (g & 1) ? e1 : e0;
        }
    }
    if (tid < 8) sums[tid] = 0;
    const int pitch = Wq + 2;
    for (int i = tid; i < 2 * (GR_FIN_ROWS + 2) * pitch; i += GR_FIN_THREADS) {
        const int side = i / ((GR_FIN_ROWS + 2) * pitch), j = i - side * (GR_FIN_ROWS + 2) * pitch, r = j / pitch, col = j - r * pitch;
        const int y = y0 - 1 + r, xw = col - 1;
        u64 v = 0;
        if (side < nsides && y >= 0 && y < H && xw >= 0 && xw < Wq) {
            const size_t o = (((size_t)n * 2 + side) * H + y) * Wq + xw;
            v = x1[o];
            if (ep[side]) v |= ep[side][o];
        }
        bw[side][r][col] = v;
    }
    __syncthreads();
    for (int i = tid; i < 2 * GR_FIN_ROWS * Wq; i += GR_FIN_THREADS) {
        const int side = i / (GR_FIN_ROWS * Wq), j = i - side * GR_FIN_ROWS * Wq, r = j / Wq, xw = j - r * Wq;
        u64 w[3];
#pragma unroll
        for (int k = 0; k < 3; ++k)   // one pixel of the word to the left, the word, one pixel of the word to the right
            w[k] = (bw[side][r + k][xw] >> (GR_CORE - 1)) | (bw[side][r + k][xw + 1] << 1) | (bw[side][r + k][xw + 2] << (GR_CORE + 1));
        const GrNodes k = gr_nodes(w[0], w[1], w[2]);
        const u64 c = y0 + r < H ? w[1] : 0;
        const u64 none = ~(k.n8.b0 | k.n8.b1 | k.n8.hi);
        const u64 end = c & ~(k.X.b1 | k.X.hi) & ~k.n8.hi;
        const u64 b = (c >> 1) & GR_COREBITS, ends = ((end & ~none) >> 1) & GR_COREBITS, iso = ((end & none) >> 1) & GR_COREBITS;
        const u64 junc = ((c & (k.X.hi | (k.X.b1 & k.X.b0))) >> 1) & GR_COREBITS;
        ow[side][0][r][xw] = b;
        ow[side][1][r][xw] = junc;
        if (acc) {
            const unsigned kb = __popcll(b), ke = __popcll(ends), ki = __popcll(iso), kj = __popcll(junc);
            if (kb) atomicAdd(&sums[side * 4 + 0], kb);
            if (ke) atomicAdd(&sums[side * 4 + 1], ke);
            if (ki) atomicAdd(&sums[side * 4 + 2], ki);
            if (kj) atomicAdd(&sums[side * 4 + 3], kj);
        }
    }
    __syncthreads();
    const int rows = min(GR_FIN_ROWS, H - y0);
    for (int r = 0; r < rows; ++r) {
        const size_t row = ((size_t)n * H + y0 + r) * W;
        for (int x = tid; x < W; x += GR_FIN_THREADS) {
            if (out_pred) out_pred[row + x] = br::pixel<GR_CORE>(ow[0][0][r], x) ? 1.0f : 0.0f;
            if (junc_pred) junc_pred[row + x] = br::pixel<GR_CORE>(ow[0][1][r], x) ? 1.0f : 0.0f;
            if (LAB && (out_true || junc_true)) {
                const int64_t l = labels[row + x];   // (read before the same thread writes it: out_true may be labels)
                const bool counted = l == 0 || l == 1;
                if (junc_true) junc_true[row + x] = counted ? (int64_t)br::pixel<GR_CORE>(ow[1][1][r], x) : l;
                if (out_true) out_true[row + x] = counted ? (int64_t)br::pixel<GR_CORE>(ow[1][0][r], x) : l;
            }
        }
    }
    if (acc && tid < 8 && sums[tid]) atomicAdd(&acc[tid], (u64)sums[tid]);
}

inline int gr_delete_launches(int L) { return (L + GR_R - 1) / GR_R; }
inline int gr_regrow_launches(int L) { return L ? (L + 1 + GR_R - 1) / GR_R : 0; }
}  // namespace

size_t gr_ws_bytes(int N, int H, int W, int min_branch) {
    return (min_branch ? 5 : 1) * br::plane_words<GR_CORE>(N, H, W) * sizeof(u64) +
           br::counter_bytes((size_t)(gr_delete_launches(min_branch) + gr_regrow_launches(min_branch)) * N * 2);
}

hipError_t gr_skeleton_graph(const float* prob, float threshold, const int64_t* labels, int min_branch, float* out_pred, int64_t* out_true,
                             float* junc_pred, int64_t* junc_true, unsigned long long* acc, void* ws, int N, int H, int W, hipStream_t st) {
    const int Wq = br::wq<GR_CORE>(W), L = min_branch, D = gr_delete_launches(L), G = gr_regrow_launches(L), nsides = labels ? 2 : 1;
    const size_t words = br::plane_words<GR_CORE>(N, H, W);
    u64* plane_o = (u64*)ws;
    u64* px[2] = {plane_o + words, plane_o + 2 * words};
    u64* pe[2] = {plane_o + 3 * words, plane_o + 4 * words};
    uint32_t* counters = (uint32_t*)(plane_o + 5 * words);   // (used with L > 0 only)
    hipLaunchKernelGGL(labels ? k_graph_init<true> : k_graph_init<false>, dim3(N * H), dim3(GR_INIT_THREADS), 0, st, prob, threshold, labels,
                       plane_o, L ? px[0] : (u64*)nullptr, counters, D + G, N, H, W, Wq);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int ntiles = (H + GR_CROWS - 1) / GR_CROWS;
    const dim3 grid(N * nsides * ntiles * Wq);
    const size_t per = (size_t)N * 2;
    for (int s = 0; s < D; ++s) {
        const int rounds = s + 1 < D ? GR_R : L - s * GR_R;
        hipLaunchKernelGGL(k_graph_delete, grid, dim3(GR_ROWS), 0, st, (const u64*)px[s & 1], px[(s + 1) & 1],
                           s ? (const uint32_t*)(counters + (s - 1) * per) : (const uint32_t*)nullptr, counters + s * per, H, Wq, rounds, nsides,
                           ntiles);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    int left = L;
    for (int g = 0; g < G; ++g) {
        const int rounds = left < (g ? GR_R : GR_R - 1) ? left : (g ? GR_R : GR_R - 1);
        left -= rounds;
        const uint32_t* prev = counters + (D + g - 1) * per;
        if (g == 0)
            hipLaunchKernelGGL(k_graph_regrow<true>, grid, dim3(GR_ROWS), 0, st, (const u64*)px[D & 1], (const u64*)plane_o, pe[0], prev,
                               counters + (D + g) * per, H, Wq, rounds, nsides, ntiles);
        else
            hipLaunchKernelGGL(k_graph_regrow<false>, grid, dim3(GR_ROWS), 0, st, (const u64*)pe[(g - 1) & 1], (const u64*)plane_o, pe[g & 1], prev,
                               counters + (D + g) * per, H, Wq, rounds, nsides, ntiles);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const int nblk = (H + GR_FIN_ROWS - 1) / GR_FIN_ROWS;
    const dim3 fgrid(N * nblk);
    const u64* x1 = L ? px[D & 1] : plane_o;
    const uint32_t* cn = L ? counters : nullptr;
    hipLaunchKernelGGL(labels ? k_graph_final<true> : k_graph_final<false>, fgrid, dim3(GR_FIN_THREADS), 0, st, x1, (const u64*)pe[0],
                       (const u64*)pe[1], cn, D, G, labels, out_pred, out_true, junc_pred, junc_true, (u64*)acc, N, H, W, Wq, nblk);
    return hipGetLastError();
}
