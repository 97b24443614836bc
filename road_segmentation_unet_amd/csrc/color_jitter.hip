// Per-sample colour jitter and noise behind the batch loader (rsu.h rsu_color_jitter): out = clamp(A x + K mean(x) + sigma g) per pixel,
// with a 3x3 matrix A, a 3x3 weight K of the sample's own channel means, and a counter-based noise field, all per sample. Contrast needs the
// mean of the finished window, so this cannot ride in the loader's store: it is a reduction and an apply pass over the batch, both bound by
// HBM. A sample's record travels as a kernel argument (no device table, no copy, no synchronisation), at most CJ_MAX_LAUNCH per launch.
//
//   k_jitter_sums   grid (ceil(S*S / CJ_CHUNK), records of the launch), 256 lanes. A workgroup reduces its CJ_CHUNK = 4096 pixels of one
//                   sample (80 workgroups per 572^2 sample: a batch of 4 gives 320, more than the 256 CUs) to three int64 sums of the
//                   channels' values in 2^-24 fixed point: 16 pixels per lane as 12-byte loads, per-lane int64 accumulators, a wave
//                   shuffle of the two 32-bit halves, LDS across the four waves, then three 8-byte stores to ws[record][chunk][3]. No
//                   atomics, nothing zeroed. Integer sums do not depend on the order, so the partition is free. Workgroups of a record
//                   whose k[] is all zero return at once (bit `record` of kmask); the launch is not issued when kmask is zero.
//   k_jitter_apply  the same grid and the same 16 pixels per lane. A workgroup first adds up its record's ceil(S*S / 4096) partial triples
//                   (each lane a stride of them, then the same wave and LDS reduction; 1.9 KB from L2 at S = 572 against the 96 KB of
//                   pixels it then moves), forms the three means, and applies the rule in place. A LANE OWNS WHOLE PIXELS: every output
//                   channel needs all three input channels and the update is in place, so a lane loads a 12-byte pixel
//                   (global_load_dwordx3), and stores it back; a wave's accesses cover 768 contiguous bytes. All 16 loads are issued
//                   before the first store. (The form of four pixels per lane as three 16-byte accesses was not built or timed.)
//
// Every float32 operation is rounded on its own (contraction off: the pragma below, and the Makefile compiles this file with
// -ffp-contract=off), in the order rsu.h states, so that hostio.color_jitter restates them in numpy bit for bit.
#include "color_jitter.h"

namespace {

struct CjLaunch {
    CjRec r[CJ_MAX_LAUNCH];
};
static_assert(sizeof(CjRec) == 80 && sizeof(CjLaunch) == 2560, "records are 80 bytes, a launch carries 2.5 KB of them");
constexpr int CJ_PER_LANE = CJ_CHUNK / 256;

struct __attribute__((packed, aligned(4))) CjPix {
    float c[3];
};

__device__ __forceinline__ long long cj_shfl_down64(long long v, int d) {
    const int lo = __shfl_down((int)(unsigned)(unsigned long long)v, d, 64);
    const int hi = __shfl_down((int)(unsigned)((unsigned long long)v >> 32), d, 64);
    return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo);
}

// s[c] of every lane of the 256-lane workgroup -> the workgroup's totals, in every lane (integers: no order to fix). One call per kernel.
__device__ __forceinline__ void cj_block_sum3(long long (&s)[3], long long (*lds)[3]) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) s[c] += cj_shfl_down64(s[c], d);
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int c = 0; c < 3; ++c) lds[threadIdx.x >> 6][c] = s[c];
    }
    __syncthreads();
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] = (lds[0][c] + lds[1][c]) + (lds[2][c] + lds[3][c]);
}

// a value in 2^-24 fixed point, saturated at +-256 (exact for every float32 in [2^-24, 256] with at most 24 - e fraction bits; rounded otherwise)
__device__ __forceinline__ long long cj_q(float v) {
#pragma clang fp contract(off)
    return (long long)rintf(fminf(fmaxf(v, -256.f), 256.f) * 16777216.f);
}

__global__ void __launch_bounds__(256) k_jitter_sums(const float* __restrict__ x, long long* __restrict__ ws, int npix, int nchunk, unsigned kmask) {
    if (!((kmask >> blockIdx.y) & 1u)) return;   // (the whole workgroup: a record without contrast needs no means)
    __shared__ long long lds[4][3];
    const CjPix* px = (const CjPix*)x + (size_t)blockIdx.y * npix;
    const int base = blockIdx.x * CJ_CHUNK + threadIdx.x;
    long long s[3] = {0, 0, 0};
#pragma unroll
    for (int i = 0; i < CJ_PER_LANE; ++i) {
        const int p = base + i * 256;
        if (p < npix) {
            const CjPix v = px[p];
#pragma unroll
            for (int c = 0; c < 3; ++c) s[c] += cj_q(v.c[c]);
        }
    }
    cj_block_sum3(s, lds);
    if (threadIdx.x < 3)
        ws[((size_t)blockIdx.y * nchunk + blockIdx.x) * 3 + threadIdx.x] = threadIdx.x == 0 ? s[0] : threadIdx.x == 1 ? s[1] : s[2];
}

__global__ void __launch_bounds__(256) k_jitter_apply(const CjLaunch a, float* x, const long long* __restrict__ ws, int npix, int nchunk,
                                                      unsigned kmask) {
#pragma clang fp contract(off)
    const CjRec r = a.r[blockIdx.y];
    float d[3] = {0.f, 0.f, 0.f};
    if ((kmask >> blockIdx.y) & 1u) {   // (the whole workgroup)
        __shared__ long long lds[4][3];
        const long long* w = ws + (size_t)blockIdx.y * nchunk * 3;
        long long s[3] = {0, 0, 0};
        for (int b = threadIdx.x; b < nchunk; b += 256) {
#pragma unroll
            for (int c = 0; c < 3; ++c) s[c] += w[(size_t)b * 3 + c];
        }
        cj_block_sum3(s, lds);
        const double den = (double)npix * 16777216.0;
        float m[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) m[c] = (float)((double)s[c] / den);
#pragma unroll
        for (int c = 0; c < 3; ++c) d[c] = (r.k[3 * c] * m[0] + r.k[3 * c + 1] * m[1]) + r.k[3 * c + 2] * m[2];
    }
    CjPix* px = (CjPix*)x + (size_t)blockIdx.y * npix;
    const int base = blockIdx.x * CJ_CHUNK + threadIdx.x;
    const bool noisy = r.sigma > 0.f;
    CjPix v[CJ_PER_LANE];
#pragma unroll
    for (int i = 0; i < CJ_PER_LANE; ++i) {
        const int p = base + i * 256;
        if (p < npix) v[i] = px[p];
    }
#pragma unroll
    for (int i = 0; i < CJ_PER_LANE; ++i) {
        const int p = base + i * 256;
        if (p < npix) {
            CjPix o;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                float y = ((r.a[3 * c] * v[i].c[0] + r.a[3 * c + 1] * v[i].c[1]) + r.a[3 * c + 2] * v[i].c[2]) + d[c];
                if (noisy) y = y + r.sigma * cj_noise(3u * (unsigned)p + (unsigned)c, r.key);
                o.c[c] = fminf(fmaxf(y, 0.f), 1.f);
            }
            px[p] = o;
        }
    }
}

}  // namespace

size_t cj_ws_bytes(int nrec, int S) {
    return (size_t)(nrec < CJ_MAX_LAUNCH ? nrec : CJ_MAX_LAUNCH) * cj_chunks(S) * 3 * sizeof(long long);
}

hipError_t cj_color_jitter(float* x, const CjRec* recs, int nrec, int S, void* ws, hipStream_t st) {
    const int npix = S * S, nchunk = cj_chunks(S);
    for (int r0 = 0; r0 < nrec; r0 += CJ_MAX_LAUNCH) {
        const int n = nrec - r0 < CJ_MAX_LAUNCH ? nrec - r0 : CJ_MAX_LAUNCH;
        CjLaunch a = {};
        unsigned kmask = 0;
        for (int k = 0; k < n; ++k) {
            a.r[k] = recs[r0 + k];
            if (cj_has_k(a.r[k])) kmask |= 1u << k;
        }
        float* xs = x + (size_t)r0 * npix * 3;
        if (kmask) {   // (ws is not null then: the entry point has checked it)
            hipLaunchKernelGGL(k_jitter_sums, dim3(nchunk, n), dim3(256), 0, st, xs, (long long*)ws, npix, nchunk, kmask);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
        hipLaunchKernelGGL(k_jitter_apply, dim3(nchunk, n), dim3(256), 0, st, a, xs, (const long long*)ws, npix, nchunk, kmask);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
