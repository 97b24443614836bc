// The border-distance weight map of the loss (rsu.h rsu_border_map): per label tile, the exact squared Euclidean distance of every valid
// pixel to the nearest valid pixel of the other class, by the separable transform in integer arithmetic, and the U-Net paper's weight
// 1 + w0 exp(-D2 / (2 sigma^2)) from it. Two launches, no atomics, no floating-point reduction: every output is a pure function of the tile.
//
//   k_border_cols  edt.h's column pass over the two class masks (coalesced 8-byte label loads): g0 | g1 << 16, the vertical distances to
//                  class 0 / class 1.
//   k_border_rows  edt.h's row pass, every pixel against the OTHER class. A row without any finite distance to a class (an
//                  all-background tile, the padding tiles of a validation pass) skips the scans for that class altogether.
#include "border_map.h"
#include "edt.h"

// Every float32 operation below must be rounded on its own: the host mirror restates them one by one. hipcc contracts a * b + c into one
// fma, also through __fmul_rn / __fadd_rn and under `#pragma clang fp contract(off)`: the Makefile compiles this file with
// -ffp-contract=off (tests/test_border_map_host.py reads the ISA for fused forms).

namespace {

constexpr int BM_INF = 0x7fffffff;      // rsu.h RSU_BORDER_D2_INF

// exp(t) for t <= 0 in float32 with a FIXED sequence of IEEE operations (no contraction, no library call), so that the host mirror
// (hostio.border_weight_map) reproduces every bit: k = rint(t log2 e), r = t - k ln2 (two steps), the degree-7 Taylor polynomial of
// exp(r) by Horner's rule, times 2^k. Below -87 the result is 0 (1 + w0 * it rounds to 1 anyway). About 2 ulp from the true value.
__device__ __forceinline__ float bm_exp(float t) {
    if (t < -87.0f) return 0.0f;
    const float k = rintf(__fmul_rn(t, __uint_as_float(0x3fb8aa3bu)));                                  // log2(e)
    float r = __fsub_rn(t, __fmul_rn(k, __uint_as_float(0x3f317200u)));                                 // ln2, high part (k * it is exact)
    r = __fsub_rn(r, __fmul_rn(k, __uint_as_float(0x35bfbe8eu)));                                       // ln2, low part
    float p = __uint_as_float(0x39500d01u);                                                             // 1/5040
    p = __fadd_rn(__fmul_rn(p, r), __uint_as_float(0x3ab60b61u));                                       // 1/720
    p = __fadd_rn(__fmul_rn(p, r), __uint_as_float(0x3c088889u));                                       // 1/120
    p = __fadd_rn(__fmul_rn(p, r), __uint_as_float(0x3d2aaaabu));                                       // 1/24
    p = __fadd_rn(__fmul_rn(p, r), __uint_as_float(0x3e2aaaabu));                                       // 1/6
    p = __fadd_rn(__fmul_rn(p, r), 0.5f);
    p = __fadd_rn(__fmul_rn(p, r), 1.0f);
    p = __fadd_rn(__fmul_rn(p, r), 1.0f);
    return __fmul_rn(p, __uint_as_float((unsigned)((int)k + 127) << 23));                               // k >= -126: a normal number
}

// grid N * nstrips (nstrips = ceil(W / 64)), block (64, ceil(H / 64)); LDS int [4][blockDim.y][64]
__global__ void __launch_bounds__(1024) k_border_cols(const int64_t* __restrict__ labels, uint32_t* __restrict__ ws, int H, int W, int nstrips) {
    extern __shared__ int bm_lds[];
    const int tx = threadIdx.x, k = threadIdx.y;
    const int n = blockIdx.x / nstrips;
    const int x = (blockIdx.x - n * nstrips) * 64 + tx, y0 = k * 64;
    const bool xin = x < W;
    const size_t img = (size_t)n * H * W;
    const int xc = xin ? x : W - 1;   // (out-of-tile lanes and rows load a valid address and drop the value: the loads stay unconditional)
    unsigned long long m0 = 0, m1 = 0;
#pragma unroll 1
    for (int i0 = 0; i0 < 64; i0 += 16) {   // 16 independent loads in flight per thread (all 64 at once would spill at 1024 threads)
        int64_t l[16];
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int y = y0 + i0 + j;
            l[j] = labels[img + (size_t)(y < H ? y : H - 1) * W + xc];
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const bool in = xin && y0 + i0 + j < H;
            m0 |= (unsigned long long)(in && l[j] == 0) << (i0 + j);
            m1 |= (unsigned long long)(in && l[j] == 1) << (i0 + j);
        }
    }
    edt_cols_store(m0, m1, bm_lds, ws, img, x, H, W);
}

// grid N * H (one workgroup per row), block a multiple of 64; LDS int [2][Wp], Wp = W rounded up to 32 (lanes that read different classes then never share a bank)
__global__ void __launch_bounds__(512) k_border_rows(const uint32_t* __restrict__ ws, const float* __restrict__ mul, float* __restrict__ out,
                                                     int32_t* __restrict__ d2out, int W, int Wp, float w0, float neg_inv_2s2) {
    extern __shared__ int bm_lds[];
    const size_t row = (size_t)blockIdx.x * W;
    const int any = edt_stage(ws, row, bm_lds, W, Wp, blockDim.x);   // bit c: some column of this row has a pixel of class c
    for (int x = threadIdx.x; x < W; x += blockDim.x) {
        const int cls = bm_lds[x] == 0 ? 0 : (bm_lds[Wp + x] == 0 ? 1 : 2);   // distance 0 to a class: the pixel has it; neither: ignored
        int d2 = BM_INF;
        float o = 0.0f;
        if (cls < 2) {
            const int best = edt_scan(bm_lds + (cls ? 0 : Wp), x, W, (any >> (1 - cls)) & 1);
            float border = 1.0f;
            if (best < EDT_BIG) {
                d2 = best;
                border = __fadd_rn(1.0f, __fmul_rn(w0, bm_exp(__fmul_rn((float)d2, neg_inv_2s2))));
            }
            o = mul ? __fmul_rn(mul[row + x], border) : border;   // (an ignored pixel's mul is never loaded)
        }
        out[row + x] = o;
        if (d2out) d2out[row + x] = d2;
    }
}

}  // namespace

size_t bm_ws_bytes(int N, int H, int W) { return (size_t)N * H * W * sizeof(uint32_t); }

hipError_t bm_border_map(const int64_t* labels, const float* mul, float* out, int32_t* d2, void* ws, int N, int H, int W, float w0,
                         float neg_inv_2s2, hipStream_t st) {
    const int CH = (H + 63) / 64, Wp = (W + 31) / 32 * 32, nstrips = (W + 63) / 64;
    hipLaunchKernelGGL(k_border_cols, dim3(N * nstrips), dim3(64, CH), (size_t)4 * CH * 64 * sizeof(int), st, labels, (uint32_t*)ws, H, W, nstrips);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int threads = nstrips * 64 < 512 ? nstrips * 64 : 512;
    hipLaunchKernelGGL(k_border_rows, dim3(N * H), dim3(threads), (size_t)2 * Wp * sizeof(int), st, (const uint32_t*)ws, mul, out, d2, W, Wp, w0,
                       neg_inv_2s2);
    return hipGetLastError();
}
