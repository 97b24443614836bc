// Device code shared by elementwise.hip and loss.hip: the 8 x bf16 pack / unpack of a 16-byte access and the stages of the opt-in head
// family (k_head_loss<DICE>, k_head_sums<EVAL> in elementwise.hip; k_head_focal<DICE>, k_head_sums_focal in loss.hip). Every function is
// static and force-inlined: each translation unit gets its own copy, nothing is linked.
#pragma once
#include "rsu_common.h"

static __device__ __forceinline__ void unpack8(const u32x4 v, float* f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[2 * i] = bf_lo(v[i]);
        f[2 * i + 1] = bf_hi(v[i]);
    }
}
static __device__ __forceinline__ u32x4 pack8(const float* f) {
    u32x4 r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r[i] = pack_bf2(f[2 * i], f[2 * i + 1]);
    return r;
}

// ---- the opt-in family: stages shared by k_head_loss<DICE> and k_head_sums<EVAL> (see the head of this section) ----
// per-thread setup: the thread's 8 channels of both weight columns and the two biases
static __device__ __forceinline__ void head_setup(const float* __restrict__ w, const float* __restrict__ b, int sub, float (&w0)[8], float (&w1)[8],
                                                  float& b0, float& b1) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        w0[i] = w[(sub * 8 + i) * 2];
        w1[i] = w[(sub * 8 + i) * 2 + 1];
    }
    b0 = b[0];
    b1 = b[1];
}
// HU pixels per thread and trip as in k_head; the pixel's 64-bit label and its weight are requested with its activations, before any is used
constexpr int HEAD_HU = 4;
template <typename IT>
static __device__ __forceinline__ void head_load(const bf16_t* __restrict__ act, const int64_t* __restrict__ labels, const float* __restrict__ pixel_w,
                                                 IT it0, IT niter, long npix, int C, int LP, int sub, int ppb, long (&pp)[HEAD_HU],
                                                 bool (&okk)[HEAD_HU], u32x4 (&raw)[HEAD_HU], int64_t (&labv)[HEAD_HU], float (&pwv)[HEAD_HU]) {
#pragma unroll
    for (int u = 0; u < HEAD_HU; ++u) {
        pp[u] = ((long)(it0 + u) * gridDim.x + blockIdx.x) * ppb + threadIdx.x / LP;
        okk[u] = (it0 + u < niter) && pp[u] < npix;
        raw[u] = okk[u] ? *(const u32x4*)(act + pp[u] * C + sub * 8) : u32x4{0u, 0u, 0u, 0u};
        labv[u] = okk[u] ? labels[pp[u]] : 0;
        pwv[u] = (okk[u] && pixel_w) ? pixel_w[pp[u]] : 1.f;
    }
}
// logits (partial dot products met with wave shuffles) and the two-way softmax: k_head's expressions, so prob gets its bits
static __device__ __forceinline__ void head_softmax(const u32x4 raw, const float (&w0)[8], const float (&w1)[8], float b0, float b1, int LP,
                                                    float (&a)[8], float& l0, float& l1, float& m, float& s, float& p0, float& p1) {
    unpack8(raw, a);
    l0 = 0.f;
    l1 = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        l0 = fmaf(a[i], w0[i], l0);
        l1 = fmaf(a[i], w1[i], l1);
    }
    for (int o = 1; o < LP; o <<= 1) {
        l0 += __shfl_xor(l0, o);
        l1 += __shfl_xor(l1, o);
    }
    l0 += b0;
    l1 += b1;
    m = fmaxf(l0, l1);
    const float e0 = expf(l0 - m), e1 = expf(l1 - m);
    s = e0 + e1;
    p1 = e1 / s;
    p0 = e0 / s;
}
// block reduce over rows of NV floats, one row per thread (an odd NV keeps the rows on different LDS banks): value j of the threads that
// hold channel group sg, in the order of their pixels
template <int NV>
static __device__ __forceinline__ float head_block_sum(const float* red, int sg, int j, int ppb, int LP) {
    float t = 0.f;
    for (int q = 0; q < ppb; ++q) t += red[(q * LP + sg) * NV + j];
    return t;
}
// k_head_final's sum of output o over the blocks' partials: lane l adds partials l, l + 64, ... (independent loads), then a fixed-order butterfly
static __device__ __forceinline__ float head_final_sum(const float* __restrict__ partial, int nblk, int nout, int o, int lane) {
    float t = 0.f;
    for (int bk = lane; bk < nblk; bk += 64) t += partial[(long)bk * nout + o];
    for (int m = 32; m > 0; m >>= 1) t += __shfl_xor(t, m);
    return t;
}
