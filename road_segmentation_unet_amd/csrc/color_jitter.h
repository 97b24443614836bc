// Launch prototypes of the per-sample colour jitter (color_jitter.hip; rsu.h rsu_color_jitter).
#pragma once
#include "rsu_common.h"

constexpr int CJ_MAX_LAUNCH = 32;   // records per launch (rsu.h RSU_JITTER_MAX_LAUNCH): they travel as kernel arguments
constexpr int CJ_CHUNK = 4096;      // pixels of a sample per workgroup, in both kernels: one triple of partial sums per chunk
// one sample: rsu.h rsu_jitter_t, field for field
struct CjRec {
    float a[9];
    float k[9];
    float sigma;
    unsigned key;
};
inline int cj_chunks(int S) { return (int)(((long)S * S + CJ_CHUNK - 1) / CJ_CHUNK); }
inline bool cj_has_k(const CjRec& r) {
    for (int i = 0; i < 9; ++i)
        if (r.k[i] != 0.f) return true;
    return false;
}
// bytes of the partial sums of one launch: int64 [min(nrec, CJ_MAX_LAUNCH)][cj_chunks(S)][3]
size_t cj_ws_bytes(int nrec, int S);
// recs: a HOST pointer; cut into launches of at most CJ_MAX_LAUNCH records on `st`; ws may be null when no record has a non-zero k[]
hipError_t cj_color_jitter(float* x, const CjRec* recs, int nrec, int S, void* ws, hipStream_t st);

// rsu.h rsu_color_jitter's hash and noise value; the loader's elastic lattice (affine_patches.hip) draws its control points from the same
__device__ __forceinline__ unsigned cj_mix(unsigned v) {
    v ^= v >> 16;
    v *= 0x85ebca6bu;
    v ^= v >> 13;
    v *= 0xc2b2ae35u;
    v ^= v >> 16;
    return v;
}

// the unit-variance noise value of element e under `key`: an Irwin-Hall sum of four 16-bit uniforms, centred and scaled
__device__ __forceinline__ float cj_noise(unsigned e, unsigned key) {
#pragma clang fp contract(off)
    const unsigned h1 = cj_mix(e ^ key), h2 = cj_mix(h1 ^ 0x9e3779b9u);
    const unsigned n = (h1 & 0xffffu) + (h1 >> 16) + (h2 & 0xffffu) + (h2 >> 16);
    return ((float)n - 131070.f) * __uint_as_float(0x37ddb3d7u);
}
