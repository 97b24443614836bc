// The one-launch batch loader (rsu.h rsu_affine_patches): cuts a batch's input windows and label patches out of the resident training
// images, each sample through a 2x2 matrix of its own about its window's centre -- bilinear taps, every tap reflected on its own about the
// edges of the ORIGINAL image. The plain window cut, the eight D4 symmetries and continuous rotation and zoom are one kernel; a sample's
// records travel as kernel arguments (no device table, no copy, no synchronisation), at most AP_MAX_LAUNCH of them per launch.
//
//   k_affine_patches  grid (ceil(S*S / 256) + ceil(P*P / 256), records of the launch), 256 lanes. The first ceil(S*S / 256) workgroups of
//                     a record write its input window, ONE LANE PER OUTPUT PIXEL: the lane forms the pixel's source coordinate once,
//                     loads its four taps as 12-byte pixels (global_load_dwordx3) and stores one 12-byte pixel; a wave's stores cover 768
//                     contiguous bytes. The other workgroups write the label patch, one lane per label (four byte taps, one 8-byte store).
//                     Lane per pixel was kept over a lane per 16 bytes of the flattened [S*S*3] row: this is a gather, four tap loads
//                     behind one coordinate per pixel, and a 16-byte lane straddles two pixels -- it would form two coordinates and
//                     fetch up to eight taps to widen nothing but the store. (The 16-byte form was not built or timed.)
//
// Every float32 operation is rounded on its own (contraction off: the pragma below, and the Makefile compiles this file with
// -ffp-contract=off), in the order rsu.h states, so that hostio.affine_patches restates them in numpy bit for bit. A sample's output is a
// pure function of its record: nothing depends on the other records of the launch or on where the record list is cut.
#include "affine_patches.h"

namespace {

struct ApLaunch {
    ApRec r[AP_MAX_LAUNCH];
};
static_assert(sizeof(ApRec) == 32 && sizeof(ApLaunch) == 1024, "records are 32 bytes, a launch carries 1 KB of them");

struct __attribute__((packed, aligned(4))) ApPix {
    float c[3];
};

// t reflected into [0, H) about the image's edges (-1 -> 0, H -> H - 1; numpy's "symmetric" padding, repeated): the tap t and the tap t + 1
__device__ __forceinline__ void ap_reflect2(int t, int H, int& r0, int& r1) {
    const int H2 = 2 * H;
    int m = t;
    if ((unsigned)t >= (unsigned)H2) {   // (a window inside the first period skips the division)
        m = t % H2;
        if (m < 0) m += H2;
    }
    const int m1 = m + 1 == H2 ? 0 : m + 1;
    r0 = m < H ? m : H2 - 1 - m;
    r1 = m1 < H ? m1 : H2 - 1 - m1;
}

// output pixel (i, j) of a [n][n] output centred at c = (n - 1) / 2: the four reflected taps and the two fractions
__device__ __forceinline__ void ap_source(const ApRec& r, float off, float c, int i, int j, int Hl, int& y0, int& y1, int& x0, int& x1, float& fy,
                                          float& fx) {
#pragma clang fp contract(off)
    const float di = (float)i - c, dj = (float)j - c;
    const float sy = (r.cy - off) + (r.m00 * di + r.m01 * dj);
    const float sx = (r.cx - off) + (r.m10 * di + r.m11 * dj);
    const float ty = floorf(sy), tx = floorf(sx);
    fy = sy - ty;
    fx = sx - tx;
    ap_reflect2((int)ty, Hl, y0, y1);
    ap_reflect2((int)tx, Hl, x0, x1);
}

__device__ __forceinline__ float ap_lerp(float v00, float v01, float v10, float v11, float fx, float gx, float fy, float gy) {
#pragma clang fp contract(off)
    return (v00 * gx + v01 * fx) * gy + (v10 * gx + v11 * fx) * fy;
}

__global__ void __launch_bounds__(256) k_affine_patches(const ApLaunch a, const float* __restrict__ images, const uint8_t* __restrict__ labels,
                                                        float* __restrict__ x_out, int64_t* __restrict__ labels_out, int He, int Hl, int S, int P,
                                                        int nbx) {
#pragma clang fp contract(off)
    const ApRec r = a.r[blockIdx.y];
    const int offset = (He - Hl) >> 1;
    const float off = (float)offset;
    int y0, y1, x0, x1;
    float fy, fx;
    if ((int)blockIdx.x < nbx) {
        const int p = blockIdx.x * 256 + threadIdx.x;
        if (p >= S * S) return;
        const int i = p / S, j = p - i * S;
        ap_source(r, off, (float)(S - 1) * 0.5f, i, j, Hl, y0, y1, x0, x1, fy, fx);
        const float gy = 1.0f - fy, gx = 1.0f - fx;
        const ApPix* img = (const ApPix*)(images + (size_t)r.image * He * He * 3);   // (the pool as a whole may exceed 2 GiB; one image does not)
        const int ra = (y0 + offset) * He + offset, rb = (y1 + offset) * He + offset;
        const ApPix v00 = img[ra + x0], v01 = img[ra + x1], v10 = img[rb + x0], v11 = img[rb + x1];
        ApPix o;
#pragma unroll
        for (int c = 0; c < 3; ++c) o.c[c] = ap_lerp(v00.c[c], v01.c[c], v10.c[c], v11.c[c], fx, gx, fy, gy);
        ((ApPix*)x_out)[(size_t)blockIdx.y * S * S + p] = o;
    } else {
        const int p = (blockIdx.x - nbx) * 256 + threadIdx.x;
        if (p >= P * P) return;
        const int i = p / P, j = p - i * P;
        ap_source(r, off, (float)(P - 1) * 0.5f, i, j, Hl, y0, y1, x0, x1, fy, fx);
        const float gy = 1.0f - fy, gx = 1.0f - fx;
        const uint8_t* lab = labels + (size_t)r.image * Hl * Hl;
        const int ra = y0 * Hl, rb = y1 * Hl;
        const float v = ap_lerp((float)lab[ra + x0], (float)lab[ra + x1], (float)lab[rb + x0], (float)lab[rb + x1], fx, gx, fy, gy);
        labels_out[(size_t)blockIdx.y * P * P + p] = v >= 0.5f ? 1 : 0;
    }
}

}  // namespace

hipError_t ap_affine_patches(const float* images, const uint8_t* labels, const ApRec* recs, int nrec, int He, int Hl, int S, int P, float* x_out,
                             int64_t* labels_out, hipStream_t st) {
    const int nbx = (S * S + 255) / 256, nbl = (P * P + 255) / 256;
    for (int r0 = 0; r0 < nrec; r0 += AP_MAX_LAUNCH) {
        const int n = nrec - r0 < AP_MAX_LAUNCH ? nrec - r0 : AP_MAX_LAUNCH;
        ApLaunch a = {};
        for (int k = 0; k < n; ++k) a.r[k] = recs[r0 + k];
        hipLaunchKernelGGL(k_affine_patches, dim3(nbx + nbl, n), dim3(256), 0, st, a, images, labels, x_out + (size_t)r0 * S * S * 3,
                           labels_out + (size_t)r0 * P * P, He, Hl, S, P, nbx);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
