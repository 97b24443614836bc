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
//   k_elastic_patches the same grid and the same lane per pixel, for rsu.h rsu_elastic_patches: a smooth displacement of the OUTPUT offset in
//                     front of the matrix. First the workgroup's 256 lanes form the record's control lattice in LDS -- (G + 3)^2 points of two
//                     floats, at most 19 * 19 * 2 = 722 floats (2.9 KB), at most three hashes per lane; nothing is stored in memory -- then
//                     one barrier; no lane returns in front of it, the lanes past the last pixel leave behind it. A lane then reads the
//                     4 x 4 control points around its pixel for both axes from LDS (neighbouring lanes read the same or neighbouring
//                     words), evaluates the cubic B-spline and goes on exactly as k_affine_patches does: ap_source_tail, ap_reflect2 and
//                     ap_lerp are the same functions. Every workgroup of a record redoes the record's hashes: 722 of them at most,
//                     against 256 x 32 LDS reads and 256 x 4 tap loads.
//
// Every float32 operation is rounded on its own (contraction off: the pragma below, and the Makefile compiles this file with
// -ffp-contract=off), in the order rsu.h states, so that hostio.affine_patches and hostio.elastic_patches restate them in numpy bit for bit. A sample's output is a
// pure function of its record: nothing depends on the other records of the launch or on where the record list is cut.
#include "affine_patches.h"
#include "color_jitter.h"   // cj_noise: the control points of the elastic lattice are the noise values of the jitter

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

// an output offset (di, dj) from the centre, through the record's matrix: the four reflected taps and the two fractions
template <class Rec>
__device__ __forceinline__ void ap_source_tail(const Rec& r, float off, float di, float dj, int Hl, int& y0, int& y1, int& x0, int& x1, float& fy,
                                               float& fx) {
#pragma clang fp contract(off)
    const float sy = (r.cy - off) + (r.m00 * di + r.m01 * dj);
    const float sx = (r.cx - off) + (r.m10 * di + r.m11 * dj);
    const float ty = floorf(sy), tx = floorf(sx);
    fy = sy - ty;
    fx = sx - tx;
    ap_reflect2((int)ty, Hl, y0, y1);
    ap_reflect2((int)tx, Hl, x0, x1);
}

// output pixel (i, j) of a [n][n] output centred at c = (n - 1) / 2
__device__ __forceinline__ void ap_source(const ApRec& r, float off, float c, int i, int j, int Hl, int& y0, int& y1, int& x0, int& x1, float& fy,
                                          float& fx) {
#pragma clang fp contract(off)
    ap_source_tail(r, off, (float)i - c, (float)j - c, Hl, y0, y1, x0, x1, fy, fx);
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

// ---- rsu.h rsu_elastic_patches ----
constexpr int EP_LATTICE_FLOATS = (EP_MAX_GRID + 3) * (EP_MAX_GRID + 3) * 2;
// the record as the kernel takes it: EpRec with q = (float)(grid / (double)S) in the first padding word
struct EpArg {
    int image;
    float cy, cx;
    float m00, m01, m10, m11;
    float alpha;
    unsigned key;
    int grid;
    float q;
    int pad_;
};
struct EpLaunch {
    EpArg r[EP_MAX_LAUNCH];
};
static_assert(sizeof(EpRec) == 48 && sizeof(EpArg) == 48 && sizeof(EpLaunch) == 1536, "records are 48 bytes, a launch carries 1.5 KB of them");

// window pixel index iw of one axis: the lattice cell k in [0, G - 1] and the four cubic B-spline weights of the fraction behind it
__device__ __forceinline__ void ep_axis(int iw, float q, int G, int& k, float (&w)[4]) {
#pragma clang fp contract(off)
    const float sixth = __uint_as_float(0x3e2aaaabu);   // 1 / 6 rounded: no division
    const float t = ((float)iw + 0.5f) * q;
    k = (int)floorf(t);
    k = k < 0 ? 0 : (k > G - 1 ? G - 1 : k);
    const float f = t - (float)k;
    const float g = 1.0f - f, f2 = f * f, f3 = f2 * f;
    w[0] = ((g * g) * g) * sixth;
    w[1] = ((3.0f * f3 - 6.0f * f2) + 4.0f) * sixth;
    w[2] = (((3.0f * f2 - 3.0f * f3) + 3.0f * f) + 1.0f) * sixth;
    w[3] = f3 * sixth;
}

// component `axis` of the field at cell (ky, kx): sum_a wy[a] * (sum_b wx[b] * c[ky + a][kx + b]), both sums in index order
__device__ __forceinline__ float ep_field(const float* lat, int n1, int ky, int kx, int axis, const float (&wy)[4], const float (&wx)[4]) {
#pragma clang fp contract(off)
    float row[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const float* c = lat + ((ky + a) * n1 + kx) * 2 + axis;
        row[a] = ((wx[0] * c[0] + wx[1] * c[2]) + wx[2] * c[4]) + wx[3] * c[6];
    }
    return ((wy[0] * row[0] + wy[1] * row[1]) + wy[2] * row[2]) + wy[3] * row[3];
}

__global__ void __launch_bounds__(256) k_elastic_patches(const EpLaunch a, const float* __restrict__ images, const uint8_t* __restrict__ labels,
                                                         float* __restrict__ x_out, int64_t* __restrict__ labels_out, int He, int Hl, int S, int P,
                                                         int nbx) {
#pragma clang fp contract(off)
    __shared__ float lat[EP_LATTICE_FLOATS];
    const EpArg r = a.r[blockIdx.y];
    const int G = r.grid, n1 = G + 3;   // (1 <= G <= EP_MAX_GRID: the launcher refuses anything else)
    for (int e = threadIdx.x; e < n1 * n1 * 2; e += 256) {
        const int pt = e >> 1, la = pt / n1, lb = pt - la * n1;
        lat[e] = r.alpha * cj_noise((unsigned)(((la * 32 + lb) << 1) | (e & 1)), r.key);
    }
    __syncthreads();   // every lane of the workgroup arrives: the lanes past the last pixel leave below, not above
    const int offset = (He - Hl) >> 1;
    const float off = (float)offset;
    const bool window = (int)blockIdx.x < nbx;
    const int n = window ? S : P, shift = window ? 0 : offset;   // a label pixel sits at (i + offset, j + offset) of the window
    const int p = (window ? blockIdx.x : blockIdx.x - nbx) * 256 + threadIdx.x;
    if (p >= n * n) return;
    const int i = p / n, j = p - i * n;
    int ky, kx, y0, y1, x0, x1;
    float wy[4], wx[4], fy, fx;
    ep_axis(i + shift, r.q, G, ky, wy);
    ep_axis(j + shift, r.q, G, kx, wx);
    const float c = (float)(n - 1) * 0.5f;
    const float di = ((float)i - c) + ep_field(lat, n1, ky, kx, 0, wy, wx);
    const float dj = ((float)j - c) + ep_field(lat, n1, ky, kx, 1, wy, wx);
    ap_source_tail(r, off, di, dj, Hl, y0, y1, x0, x1, fy, fx);
    const float gy = 1.0f - fy, gx = 1.0f - fx;
    if (window) {
        const ApPix* img = (const ApPix*)(images + (size_t)r.image * He * He * 3);
        const int ra = (y0 + offset) * He + offset, rb = (y1 + offset) * He + offset;
        const ApPix v00 = img[ra + x0], v01 = img[ra + x1], v10 = img[rb + x0], v11 = img[rb + x1];
        ApPix o;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) o.c[ch] = ap_lerp(v00.c[ch], v01.c[ch], v10.c[ch], v11.c[ch], fx, gx, fy, gy);
        ((ApPix*)x_out)[(size_t)blockIdx.y * S * S + p] = o;
    } else {
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

hipError_t ep_elastic_patches(const float* images, const uint8_t* labels, const EpRec* recs, int nrec, int He, int Hl, int S, int P, float* x_out,
                              int64_t* labels_out, hipStream_t st) {
    for (int k = 0; k < nrec; ++k)   // (the lattice in LDS has room for EP_MAX_GRID cells per axis)
        if (recs[k].grid < 1 || recs[k].grid > EP_MAX_GRID) return hipErrorInvalidValue;
    const int nbx = (S * S + 255) / 256, nbl = (P * P + 255) / 256;
    for (int r0 = 0; r0 < nrec; r0 += EP_MAX_LAUNCH) {
        const int n = nrec - r0 < EP_MAX_LAUNCH ? nrec - r0 : EP_MAX_LAUNCH;
        EpLaunch a = {};
        for (int k = 0; k < n; ++k) {
            const EpRec& r = recs[r0 + k];
            // cells per pixel, in double and rounded once: the host mirror forms the same float, and the kernel never divides
            a.r[k] = EpArg{r.image, r.cy, r.cx, r.m00, r.m01, r.m10, r.m11, r.alpha, r.key, r.grid, (float)((double)r.grid / (double)S), 0};
        }
        hipLaunchKernelGGL(k_elastic_patches, dim3(nbx + nbl, n), dim3(256), 0, st, a, images, labels, x_out + (size_t)r0 * S * S * 3,
                           labels_out + (size_t)r0 * P * P, He, Hl, S, P, nbx);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}
