// Mask distances (include/rsu_distance.h): the exact squared Euclidean distance of every pixel to the predicted mask P = {counted and
// prob >= threshold} and to the truth mask T = {label == 1}, by the separable transform in integer arithmetic, and the histogram of
// those distances over the pixels of the other mask. The transform itself is edt.h's, shared with border_map.hip; the masks are
// built from prob and labels64 directly.
//
//   k_dist_cols   edt.h's column pass (coalesced label and probability loads, 4-byte stores): gT | gP << 16.
//   k_dist_rows   edt.h's row pass. Exact int32 out.
//   k_dist_hist   DT_HIST_ROWS rows per workgroup. Nothing past the last bin is needed: the staged squares are those of min(g, 63), as
//                 16-bit words, and the scan ends by d = 62 whatever the data. Only pixels of P look up T and only pixels of T look up P;
//                 bins are counted with LDS integer atomics (the first and the last bin in registers first: most pixels land there),
//                 and one 64-bit integer atomic add per non-zero bin per workgroup goes to acc. Integer adds commute: acc is a function
//                 of the inputs alone.
#include "distance.h"
#include "edt.h"

// rows of an image per workgroup of k_dist_hist: more rows, fewer flush atomics and fewer, longer workgroups (tools/bench_distance.py
// times 1, 2, 4 and 8 from A/B builds: make VARIANT=rowsK EXTRA=-DDT_HIST_ROWS=K)
#ifndef DT_HIST_ROWS
#define DT_HIST_ROWS 4
#endif

namespace {

constexpr int DT_NONE = 0x7fffffff;     // rsu_distance.h RSU_DIST_NONE
constexpr int DT_LAST = DT_BINS - 1;    // the saturating bin
constexpr int DT_HIST_THREADS = 256;

// grid N * nstrips (nstrips = ceil(W / 64)), block (64, ceil(H / 64)); LDS int [4][blockDim.y][64]. LAB: labels given (else all counted, T empty)
template <bool LAB>
__global__ void __launch_bounds__(1024) k_dist_cols(const float* __restrict__ prob, float threshold, const int64_t* __restrict__ labels,
                                                    uint32_t* __restrict__ ws, int H, int W, int nstrips) {
    extern __shared__ int dt_lds[];
    const int tx = threadIdx.x, k = threadIdx.y;
    const int n = blockIdx.x / nstrips;
    const int x = (blockIdx.x - n * nstrips) * 64 + tx, y0 = k * 64;
    const bool xin = x < W;
    const size_t img = (size_t)n * H * W;
    const int xc = xin ? x : W - 1;   // (out-of-image lanes and rows load a valid address and drop the value: the loads stay unconditional)
    unsigned long long mt = 0, mp = 0;
#pragma unroll 1
    for (int i0 = 0; i0 < 64; i0 += 8) {   // 8 label and 8 probability loads in flight per thread
        int64_t l[8];
        float p[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int y = y0 + i0 + j;
            const size_t at = img + (size_t)(y < H ? y : H - 1) * W + xc;
            l[j] = LAB ? labels[at] : 0;
            p[j] = prob[at];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const bool in = xin && y0 + i0 + j < H;
            const bool counted = l[j] == 0 || l[j] == 1;
            mt |= (unsigned long long)(LAB && in && l[j] == 1) << (i0 + j);
            mp |= (unsigned long long)(in && counted && p[j] >= threshold) << (i0 + j);   // (NaN compares false)
        }
    }
    edt_cols_store(mt, mp, dt_lds, ws, img, x, H, W);
}

// grid N * H (one workgroup per row), block a multiple of 64; LDS int [2][Wp], Wp = W rounded up to 32
__global__ void __launch_bounds__(512) k_dist_rows(const uint32_t* __restrict__ ws, int32_t* __restrict__ d2_pred, int32_t* __restrict__ d2_true,
                                                   int W, int Wp) {
    extern __shared__ int dt_lds[];
    const size_t row = (size_t)blockIdx.x * W;
    const int any = edt_stage(ws, row, dt_lds, W, Wp, blockDim.x);   // bit 0: some column of this row has a pixel of T; bit 1: of P
    for (int x = threadIdx.x; x < W; x += blockDim.x) {
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            int32_t* out = c ? d2_pred : d2_true;
            if (!out) continue;
            const int best = edt_scan(dt_lds + c * Wp, x, W, (any >> c) & 1);
            out[row + x] = best < EDT_BIG ? best : DT_NONE;
        }
    }
}

// the smallest r with r * r >= d2, for d2 in [1, 62^2]: in integers
__device__ __forceinline__ int dt_bin(int d2) {
    int s = 0;   // the largest s with s * s < d2
#pragma unroll
    for (int b = 32; b; b >>= 1)
        if ((s + b) * (s + b) < d2) s += b;
    return s + 1;
}

// grid N * nblk (nblk = ceil(H / ROWS)), block DT_HIST_THREADS; LDS unsigned [2][DT_BINS] then unsigned short [ROWS][2][Wp] (Wp even)
template <int ROWS>
__global__ void __launch_bounds__(DT_HIST_THREADS) k_dist_hist(const uint32_t* __restrict__ ws, unsigned long long* __restrict__ acc, int H,
                                                               int W, int Wp, int nblk) {
    extern __shared__ int dt_lds[];
    unsigned* hist = (unsigned*)dt_lds;
    unsigned short* sq = (unsigned short*)(hist + 2 * DT_BINS);
    const int n = blockIdx.x / nblk, y0 = (blockIdx.x - n * nblk) * ROWS;
    const int count = min(ROWS, H - y0) * W;   // (the rows of a workgroup are contiguous in ws)
    const size_t base = ((size_t)n * H + y0) * W;
    if (threadIdx.x < 2 * DT_BINS) hist[threadIdx.x] = 0;
    for (int i = threadIdx.x; i < count; i += DT_HIST_THREADS) {
        const unsigned u = ws[base + i];
        const int r = i / W, x = i - r * W;
        const unsigned gt = min(u & 0xffffu, (unsigned)DT_LAST), gp = min(u >> 16, (unsigned)DT_LAST);   // 63^2 is past every bin below the last
        sq[(r * 2) * Wp + x] = (unsigned short)(gt * gt);
        sq[(r * 2 + 1) * Wp + x] = (unsigned short)(gp * gp);
    }
    __syncthreads();
    unsigned both = 0, last_p = 0, last_t = 0;   // pixels of P and T (bin 0 of both sides); pixels of P / of T in the last bin
    for (int i = threadIdx.x; i < count; i += DT_HIST_THREADS) {
        const int r = i / W, x = i - r * W;
        const unsigned short* rowt = sq + (r * 2) * Wp;
        const unsigned short* rowp = rowt + Wp;
        const bool in_t = rowt[x] == 0, in_p = rowp[x] == 0;
        if (!in_t && !in_p) continue;
        if (in_t && in_p) {
            ++both;
            continue;
        }
        const unsigned short* other = in_p ? rowt : rowp;
        const int side = in_p ? 0 : 1;
        const int best = edt_scan(other, x, W);   // (best <= 63^2: ends by d = 62)
        if (best > (DT_LAST - 1) * (DT_LAST - 1)) {
            last_p += in_p ? 1u : 0u;
            last_t += in_p ? 0u : 1u;
        } else
            atomicAdd(&hist[side * DT_BINS + dt_bin(best)], 1u);   // (best >= 1 here: the pixel is not in the other mask)
    }
    if (both) {
        atomicAdd(&hist[0], both);
        atomicAdd(&hist[DT_BINS], both);
    }
    if (last_p) atomicAdd(&hist[DT_LAST], last_p);
    if (last_t) atomicAdd(&hist[DT_BINS + DT_LAST], last_t);
    __syncthreads();
    if (threadIdx.x < 2 * DT_BINS && hist[threadIdx.x]) atomicAdd(&acc[threadIdx.x], (unsigned long long)hist[threadIdx.x]);
}

hipError_t dt_cols(const float* prob, float threshold, const int64_t* labels, void* ws, int N, int H, int W, hipStream_t st) {
    const int CH = (H + 63) / 64, nstrips = (W + 63) / 64;
    const size_t lds = (size_t)4 * CH * 64 * sizeof(int);
    hipLaunchKernelGGL(labels ? k_dist_cols<true> : k_dist_cols<false>, dim3(N * nstrips), dim3(64, CH), lds, st, prob, threshold, labels,
                       (uint32_t*)ws, H, W, nstrips);
    return hipGetLastError();
}

}  // namespace

size_t dt_ws_bytes(int N, int H, int W) { return (size_t)N * H * W * sizeof(uint32_t); }

hipError_t dt_mask_distance(const float* prob, float threshold, const int64_t* labels, int32_t* d2_pred, int32_t* d2_true, void* ws, int N,
                            int H, int W, hipStream_t st) {
    hipError_t e = dt_cols(prob, threshold, labels, ws, N, H, W, st);
    if (e != hipSuccess) return e;
    const int Wp = (W + 31) / 32 * 32, nstrips = (W + 63) / 64;
    const int threads = nstrips * 64 < 512 ? nstrips * 64 : 512;
    hipLaunchKernelGGL(k_dist_rows, dim3(N * H), dim3(threads), (size_t)2 * Wp * sizeof(int), st, (const uint32_t*)ws, d2_pred, d2_true, W, Wp);
    return hipGetLastError();
}

hipError_t dt_distance_hist(const float* prob, float threshold, const int64_t* labels, unsigned long long* acc, void* ws, int N, int H, int W,
                            hipStream_t st) {
    hipError_t e = dt_cols(prob, threshold, labels, ws, N, H, W, st);
    if (e != hipSuccess) return e;
    const int Wp = (W + 1) / 2 * 2, nblk = (H + DT_HIST_ROWS - 1) / DT_HIST_ROWS;
    const size_t lds = (size_t)2 * DT_BINS * sizeof(unsigned) + (size_t)DT_HIST_ROWS * 2 * Wp * sizeof(unsigned short);
    hipLaunchKernelGGL(k_dist_hist<DT_HIST_ROWS>, dim3(N * nblk), dim3(DT_HIST_THREADS), lds, st, (const uint32_t*)ws, acc, H, W, Wp, nblk);
    return hipGetLastError();
}
