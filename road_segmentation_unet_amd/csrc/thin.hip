// Mask thinning (include/rsu_thin.h): the centre-lines of the predicted mask P = {counted and prob >= threshold} and of the truth mask
// T = {label == 1} by Guo & Hall's two-sub-iteration parallel thinning, evaluated bit-sliced on bit rows.
//
// ws holds three bit planes in the layout of bitrows.h (CORE = TH_CORE). Plane O keeps the masks for the counts, planes A and B are the
// working copies: step s reads one and writes the other. Behind them sit the counters.
//
//   k_thin_init   bitrows.h's init launch. Writes planes O and A; clears the counters.
//   k_thin_step   bitrows.h's step tile: east and west are shifts of a thread's own window and north and south are its neighbours'
//                 registers, handed over through LDS (two buffers: one barrier per sub-iteration). What is shifted in at the window's
//                 rim is wrong; the error walks one pixel per sub-iteration and after 2 * TH_K of them has not left the halo. Deletions
//                 of core pixels are counted per thread and added to the launch's own counter; the launch behind reads it and returns
//                 where it is 0: that image side was at its fixed point and both planes hold it.
//   k_thin_final  TH_FIN_ROWS rows per workgroup: the bits of the last plane and of plane O to skel_pred / skel_true, the four counts to
//                 acc (LDS integer atomics, one 64-bit atomic add per non-zero count per workgroup), the last launch's count of its last
//                 iteration to info.
#include "thin.h"
#include "bitrows.h"

#ifndef TH_ROWS
#define TH_ROWS 128   // rows of a step tile, halo included: TH_ROWS - 2 * TH_HALO core rows
#endif

namespace {

namespace br = bitrows;
using br::u64;
constexpr int TH_INIT_THREADS = 256;
constexpr int TH_FIN_THREADS = 256, TH_FIN_ROWS = 4;
constexpr int TH_CROWS = TH_ROWS - 2 * TH_HALO;
constexpr u64 TH_COREBITS = (1ull << TH_CORE) - 1;
constexpr int TH_MAX_WQ = (TH_MAX_SIDE + TH_CORE - 1) / TH_CORE;
static_assert(TH_CROWS >= 1 && TH_ROWS % 64 == 0 && 4 * TH_MAX_WQ <= TH_FIN_THREADS, "tile geometry");

// grid N * H, block TH_INIT_THREADS: bitrows.h init_row. Plane A starts as a copy of plane O
template <bool LAB>
__global__ void __launch_bounds__(TH_INIT_THREADS) k_thin_init(const float* __restrict__ prob, float threshold,
                                                               const int64_t* __restrict__ labels, u64* __restrict__ plane_o,
                                                               u64* __restrict__ plane_a, uint32_t* __restrict__ counters, int nlaunch,
                                                               int N, int H, int W, int Wq) {
    br::init_row<LAB, TH_CORE, TH_INIT_THREADS, TH_MAX_SIDE>(prob, threshold, labels, plane_o, plane_a, counters, nlaunch, N, H, W, Wq);
}

// the pixels of window c that a sub-iteration deletes; u and d are the windows of the rows above and below
template <int SUB>
__device__ __forceinline__ u64 th_deleted(u64 u, u64 c, u64 d) {
    const auto [p2, p3, p4, p5, p6, p7, p8, p9] = br::ring(u, c, d);
    // C == 1: exactly one of the four terms (a two-bit adder: the pair sums are a, b and e, f)
    const u64 t1 = ~p2 & (p3 | p4), t2 = ~p4 & (p5 | p6), t3 = ~p6 & (p7 | p8), t4 = ~p8 & (p9 | p2);
    const u64 c_one = ((t1 ^ t2) ^ (t3 ^ t4)) & ~((t1 & t2) | (t3 & t4));
    // N = min(N1, N2) in {2, 3}: both sums >= 2 and not both 4
    const u64 q1 = p9 | p2, q2 = p3 | p4, q3 = p5 | p6, q4 = p7 | p8;
    const u64 r1 = p2 | p3, r2 = p4 | p5, r3 = p6 | p7, r4 = p8 | p9;
    const u64 n1_ge2 = (q1 & q2) | (q3 & q4) | ((q1 ^ q2) & (q3 ^ q4)), n1_4 = q1 & q2 & q3 & q4;
    const u64 n2_ge2 = (r1 & r2) | (r3 & r4) | ((r1 ^ r2) & (r3 ^ r4)), n2_4 = r1 & r2 & r3 & r4;
    const u64 n_ok = n1_ge2 & n2_ge2 & ~(n1_4 & n2_4);
    const u64 m = SUB == 0 ? (p6 | p7 | ~p9) & p8 : (p2 | p3 | ~p5) & p4;
    return c & c_one & n_ok & ~m;
}

// grid N * nsides * ntiles * Wq (ntiles = ceil(H / TH_CROWS)), block TH_ROWS. prev: the counters of the launch before (nullptr for the first step);
// cnt: this launch's; last: the deletions of this launch's last iteration (nullptr but for the last step). iters in [1, TH_K].
__global__ void __launch_bounds__(TH_ROWS) k_thin_step(const u64* __restrict__ in, u64* __restrict__ out, const uint32_t* __restrict__ prev,
                                                       uint32_t* __restrict__ cnt, uint32_t* __restrict__ last, int H, int Wq, int iters,
                                                       int nsides, int ntiles) {
    __shared__ u64 rows[2][TH_ROWS + 2];
    __shared__ unsigned red[2];
    const br::Tile t = br::tile_open<TH_HALO, TH_ROWS>(rows, red, prev, H, Wq, nsides, ntiles);
    if (t.skip) return;
    const int tid = threadIdx.x;
    u64 c = t.in_image ? br::window<TH_CORE, TH_HALO>(in + t.row, t.xw, Wq) : 0;
    const u64 core = TH_COREBITS << TH_HALO;
    unsigned total = 0, final_it = 0;
    for (int it = 0; it < iters; ++it) {
        unsigned here = 0;
        {
            rows[0][tid + 1] = c;
            __syncthreads();
            const u64 del = th_deleted<0>(rows[0][tid], c, rows[0][tid + 2]);
            c &= ~del;
            here += __popcll(del & core);
        }
        {
            rows[1][tid + 1] = c;
            __syncthreads();
            const u64 del = th_deleted<1>(rows[1][tid], c, rows[1][tid + 2]);
            c &= ~del;
            here += __popcll(del & core);
        }
        total += here;
        if (it == iters - 1) final_it = here;
    }
    br::tile_close<TH_CORE, TH_HALO>(t, out, c, red, total, cnt, final_it, last);
}

// grid N * nblk (nblk = ceil(H / TH_FIN_ROWS)), block TH_FIN_THREADS. fin: the plane behind the last step; last: [N][2] (see k_thin_step)
template <bool LAB>
__global__ void __launch_bounds__(TH_FIN_THREADS) k_thin_final(const u64* __restrict__ fin, const u64* __restrict__ plane_o,
                                                               const int64_t* __restrict__ labels, const uint32_t* __restrict__ last,
                                                               float* __restrict__ skel_pred, int64_t* __restrict__ skel_true,
                                                               u64* __restrict__ acc, uint32_t* __restrict__ info, int H, int W, int Wq, int nblk) {
    __shared__ u64 w[4][TH_MAX_WQ];   // the row's words: S_P, S_T, P, T
    __shared__ unsigned sums[4];
    const int tid = threadIdx.x, n = blockIdx.x / nblk, y0 = (blockIdx.x - n * nblk) * TH_FIN_ROWS;
    if (info && y0 == 0 && tid < 2) info[n * 2 + tid] = last[n * 2 + tid];   // (without labels side 1 never ran: its counter is the init's 0)
    if (tid < 4) sums[tid] = 0;
    unsigned k0 = 0, k1 = 0, k2 = 0, k3 = 0;
    const int rows = min(TH_FIN_ROWS, H - y0);
    for (int r = 0; r < rows; ++r) {
        const int y = y0 + r;
        __syncthreads();
        if (tid < 4 * Wq) {
            const int which = tid / Wq, xw = tid - which * Wq, side = which & 1;
            const u64* pl = which < 2 ? fin : plane_o;
            w[which][xw] = (LAB || !side) ? pl[(((size_t)n * 2 + side) * H + y) * Wq + xw] : 0;
        }
        __syncthreads();
        const size_t row = ((size_t)n * H + y) * W;
        for (int x = tid; x < W; x += TH_FIN_THREADS) {
            const unsigned sp = br::pixel<TH_CORE>(w[0], x), st = br::pixel<TH_CORE>(w[1], x);
            const unsigned p = br::pixel<TH_CORE>(w[2], x), t = br::pixel<TH_CORE>(w[3], x);
            if (skel_pred) skel_pred[row + x] = sp ? 1.0f : 0.0f;
            if (skel_true) {
                const int64_t l = labels[row + x];
                skel_true[row + x] = (l == 0 || l == 1) ? (int64_t)st : l;
            }
            k0 += sp;
            k1 += sp & t;
            k2 += st;
            k3 += st & p;
        }
    }
    if (!acc) return;   // (the same for the whole workgroup)
    if (k0) atomicAdd(&sums[0], k0);
    if (k1) atomicAdd(&sums[1], k1);
    if (k2) atomicAdd(&sums[2], k2);
    if (k3) atomicAdd(&sums[3], k3);
    __syncthreads();
    if (tid < 4 && sums[tid]) atomicAdd(&acc[tid], (u64)sums[tid]);
}

inline int th_steps(int max_iters) { return (max_iters + TH_K - 1) / TH_K; }

}  // namespace

// counters: one [N][2] per step launch, then the [N][2] of the last step's last iteration
size_t th_ws_bytes(int N, int H, int W, int max_iters) {
    return 3 * br::plane_words<TH_CORE>(N, H, W) * sizeof(u64) + br::counter_bytes((size_t)(th_steps(max_iters) + 1) * N * 2);
}

hipError_t th_mask_thin(const float* prob, float threshold, const int64_t* labels, int max_iters, float* skel_pred, int64_t* skel_true,
                        unsigned long long* acc, uint32_t* info, void* ws, int N, int H, int W, hipStream_t st) {
    const int Wq = br::wq<TH_CORE>(W), S = th_steps(max_iters), nsides = labels ? 2 : 1;
    const size_t words = br::plane_words<TH_CORE>(N, H, W);
    u64* plane_o = (u64*)ws;
    u64* plane[2] = {plane_o + words, plane_o + 2 * words};
    uint32_t* counters = (uint32_t*)(plane_o + 3 * words);
    uint32_t* last = counters + (size_t)S * N * 2;
    hipLaunchKernelGGL(labels ? k_thin_init<true> : k_thin_init<false>, dim3(N * H), dim3(TH_INIT_THREADS), 0, st, prob, threshold, labels,
                       plane_o, plane[0], counters, S + 1, N, H, W, Wq);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int ntiles = (H + TH_CROWS - 1) / TH_CROWS;
    const dim3 grid(N * nsides * ntiles * Wq);
    for (int s = 0; s < S; ++s) {
        const int iters = s + 1 < S ? TH_K : max_iters - s * TH_K;
        hipLaunchKernelGGL(k_thin_step, grid, dim3(TH_ROWS), 0, st, (const u64*)plane[s & 1], plane[(s + 1) & 1],
                           s ? (const uint32_t*)(counters + (size_t)(s - 1) * N * 2) : (const uint32_t*)nullptr, counters + (size_t)s * N * 2,
                           s + 1 == S ? last : (uint32_t*)nullptr, H, Wq, iters, nsides, ntiles);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    const int nblk = (H + TH_FIN_ROWS - 1) / TH_FIN_ROWS;
    hipLaunchKernelGGL(labels ? k_thin_final<true> : k_thin_final<false>, dim3(N * nblk), dim3(TH_FIN_THREADS), 0, st, (const u64*)plane[S & 1],
                       (const u64*)plane_o, labels, (const uint32_t*)last, skel_pred, skel_true, (u64*)acc, info, H, W, Wq, nblk);
    return hipGetLastError();
}
