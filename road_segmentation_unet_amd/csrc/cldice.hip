#include "cldice.h"

// The clDice term (include/rsu_cldice.h; Shit et al., CVPR 2021): scale * (1 - clD) from the soft skeletons of the prob map and of the label
// map. Per map x [H][W] (an image on its own: no window crosses into another), float32, one rounding per operation (nothing here is
// contracted into a fused multiply-add: hostio.soft_skeleton restates the maps bit for bit):
//   E_0 = x, E_{j+1} = erode(E_j) (min over the cross), O_j = dilate(E_{j+1}) (max over the 3 x 3 box), d_j = relu(E_j - O_j), j = 0..k
//   S_0 = d_0, S_j = S_{j-1} + relu(d_j - S_{j-1} d_j), skel(x) = S_k
// A framework runs this as 6 (k + 1) pooling launches per map; here the whole chain of a tile stays in LDS.
// Forward (k_cldice_fwd): one workgroup per 32 x 32 tile stages the tile and a halo of k + 2 of the map, erodes it level by level between two
// LDS buffers over a region that shrinks by one per level (E_j is exact on the tile +- (k + 2 - j)), and keeps S of its four pixels per
// thread in registers. The label map is formed from the 64-bit labels while staging. For the prob map it also leaves E_1 .. E_{k+1} and
// S_0 .. S_{k-1} of its tile in the workspace: the backward walks the levels downwards and needs each level's values when it gets there.
// Four partial sums per workgroup; k_cldice_final adds them to `sums` in a fixed order (the heads' final kernels' lanes and order).
// Backward (k_cldice_bwd): a gather, one workgroup per 16 x 16 tile of gprob. With a_j the gradient that reaches (E_j - O_j) through d_j,
//   gE_j = a_j + erode^T_{E_j}(gE_{j+1}) - dilate^T_{E_j}(a_{j-1}),   gE_{k+2} = a_{k+1} = a_{-1} = 0,   gprob = gE_0 + the direct part
// where ^T routes a window's gradient to the window's winner. Walking j = k + 1 .. 0, gE_j is needed on the tile +- j, a_{j-1} and the
// winners of the windows of E_j on the tile +- (j + 1), E_j itself on the tile +- (j + 2): the region shrinks by one per level. Each level
// stages E_j, recomputes every window's winner FROM THE VALUES into one byte per pixel (argmin in bits 0..2, argmax in bits 3..6), forms
// a_{j-1} (the pointwise recursion through S runs downwards in a map of its own) and then every pixel collects from the neighbours whose
// winner it is. Nothing is scattered, no float atomic: the order of every sum is fixed.
// Ties: among equal candidates the first in the window's row-major order wins, by strict comparisons (cross: up, left, centre, right, down);
// relu'(0) = 0. Positions outside the image are no candidates. No loop depends on data: every trip count is a function of k and the tile.
constexpr int CL_FWD_R = CL_FWD_TILE + 2 * (CL_MAX_ITERS + 2);   // 68: tile + halo, the forward's LDS pitch at k = 16
constexpr int CL_BWD_TILE = 16;
constexpr int CL_BWD_R = CL_BWD_TILE + 2 * (CL_MAX_ITERS + 3);   // 54

// the first of the existing candidates starts; a later one replaces it only if strictly smaller / greater
#define CL_MIN(ex, c, id) if ((ex) && (cm < 0 || (c) < vm)) { vm = (c); cm = (id); }
#define CL_MAX(ex, c, id) if ((ex) && (cx < 0 || (c) > vx)) { vx = (c); cx = (id); }

__global__ void __launch_bounds__(256) k_cldice_fwd(const float* __restrict__ prob, const int64_t* __restrict__ labels, int k,
                                                    float* __restrict__ skel_p, float* __restrict__ skel_y, float* __restrict__ maps,
                                                    float* __restrict__ partial, int H, int W, int tiles_x, int tiles_y, long N) {
#pragma clang fp contract(off)
    __shared__ float Ebuf[2][CL_FWD_R * CL_FWD_R];
    __shared__ float red[256 * 5];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    int t = blockIdx.x;
    const int tcx = t % tiles_x;
    t /= tiles_x;
    const int tcy = t % tiles_y, b = t / tiles_y;
    const int h = k + 2, RW = CL_FWD_TILE + 2 * h;
    const int r0 = tcy * CL_FWD_TILE - h, c0 = tcx * CL_FWD_TILE - h;
    const long img = (long)b * H * W;
    const int gc_t = tcx * CL_FWD_TILE + tx;   // the column of this thread's four tile pixels; their rows are tcy * 32 + ty + 8 u
    float Sk[2][4];
    for (int which = 0; which < 2; ++which) {   // 0: the prob map, 1: the label map
        float* Ec = Ebuf[0];
        float* En = Ebuf[1];
        for (int lr = ty; lr < RW; lr += 8) {
            const int gr = r0 + lr;
            for (int lc = tx; lc < RW; lc += 32) {
                const int gc = c0 + lc;
                float v = 0.f;
                if (gr >= 0 && gr < H && gc >= 0 && gc < W) {
                    const long g = img + (long)gr * W + gc;
                    v = which ? (labels[g] == 1 ? 1.f : 0.f) : prob[g];
                }
                Ec[lr * RW + lc] = v;
            }
        }
        __syncthreads();
        float S[4] = {0.f, 0.f, 0.f, 0.f};
        for (int j = 0; j <= k; ++j) {
            // E_{j+1} = erode(E_j) on the region less j + 1 on every side
            const int lo = j + 1, hi = RW - j - 1;
            for (int lr = lo + ty; lr < hi; lr += 8) {
                const int gr = r0 + lr;
                if (gr < 0 || gr >= H) continue;
                for (int lc = lo + tx; lc < hi; lc += 32) {
                    const int gc = c0 + lc;
                    if (gc < 0 || gc >= W) continue;
                    const float* e = Ec + lr * RW + lc;
                    float vm = 0.f;
                    int cm = -1;
                    CL_MIN(gr > 0, e[-RW], 0)
                    CL_MIN(gc > 0, e[-1], 1)
                    CL_MIN(true, e[0], 2)
                    CL_MIN(gc < W - 1, e[1], 3)
                    CL_MIN(gr < H - 1, e[RW], 4)
                    En[lr * RW + lc] = vm;
                }
            }
            __syncthreads();
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int tr = ty + 8 * u, gr = tcy * CL_FWD_TILE + tr;
                if (gr >= H || gc_t >= W) continue;
                const int li = (tr + h) * RW + tx + h;
                const float* e = En + li;
                float vx = 0.f;
                int cx = -1;
#pragma unroll
                for (int dr = -1; dr <= 1; ++dr)
#pragma unroll
                    for (int dc = -1; dc <= 1; ++dc)
                        CL_MAX(gr + dr >= 0 && gr + dr < H && gc_t + dc >= 0 && gc_t + dc < W, e[dr * RW + dc], (dr + 1) * 3 + dc + 1)
                const float df = Ec[li] - vx;
                const float d = df > 0.f ? df : 0.f;
                if (j == 0) {
                    S[u] = d;
                } else {
                    const float sd = S[u] * d;
                    const float uu = d - sd;
                    S[u] = S[u] + (uu > 0.f ? uu : 0.f);
                }
                if (which == 0) {
                    const long g = img + (long)gr * W + gc_t;
                    maps[(long)j * N + g] = e[0];                            // E_{j+1}
                    if (j < k) maps[(long)(k + 1 + j) * N + g] = S[u];       // S_j
                }
            }
            __syncthreads();   // (E_j is read above and overwritten by the next level's erosion)
            float* sw = Ec;
            Ec = En;
            En = sw;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            Sk[which][u] = S[u];
            const int gr = tcy * CL_FWD_TILE + ty + 8 * u;
            if (gr < H && gc_t < W) (which ? skel_y : skel_p)[img + (long)gr * W + gc_t] = S[u];
        }
    }
    // {A, Bp, Cc, Dy} of the tile: ignored pixels (a label that is neither 0 nor 1, all 64 bits) add nothing, by selection
    float sA = 0.f, sB = 0.f, sC = 0.f, sD = 0.f;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
        const int gr = tcy * CL_FWD_TILE + ty + 8 * u;
        if (gr >= H || gc_t >= W) continue;
        const long g = img + (long)gr * W + gc_t;
        const int64_t lab = labels[g];
        if (lab != 0 && lab != 1) continue;
        if (lab) sA += Sk[0][u];
        sB += Sk[0][u];
        sC += Sk[1][u] * prob[g];
        sD += Sk[1][u];
    }
    float* my = red + threadIdx.x * 5;
    my[0] = sA; my[1] = sB; my[2] = sC; my[3] = sD;
    __syncthreads();
    if (threadIdx.x < 4) {
        float s = 0.f;
        for (int q = 0; q < 256; ++q) s += red[q * 5 + threadIdx.x];
        partial[(long)blockIdx.x * 4 + threadIdx.x] = s;
    }
}
// one wave per sum, k_head_final's lanes and order; sums[0..3] ACCUMULATE (the caller zeroes)
__global__ void __launch_bounds__(256) k_cldice_final(const float* __restrict__ partial, float* __restrict__ sums, int nblk) {
    const int o = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const float t = head_final_sum(partial, nblk, 4, o, lane);
    if (lane == 0) sums[o] += t;
}

__global__ void __launch_bounds__(256) k_cldice_bwd(const float* __restrict__ prob, const int64_t* __restrict__ labels,
                                                    const float* __restrict__ skel_y, const float* __restrict__ sums,
                                                    const float* __restrict__ maps, int k, float scale, float smooth, float* __restrict__ gprob,
                                                    int H, int W, int tiles_x, int tiles_y, long N) {
#pragma clang fp contract(off)
    constexpr int RR = CL_BWD_R * CL_BWD_R;
    __shared__ float Eb[RR];
    __shared__ float gS[RR];
    __shared__ float bufs[3][RR];
    __shared__ unsigned char code[RR];
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    int t = blockIdx.x;
    const int tcx = t % tiles_x;
    t /= tiles_x;
    const int tcy = t % tiles_y, b = t / tiles_y;
    const int hh = k + 3, RW = CL_BWD_TILE + 2 * hh;
    const int r0 = tcy * CL_BWD_TILE - hh, c0 = tcx * CL_BWD_TILE - hh;
    const long img = (long)b * H * W;
    // the uniform factors, from the sums as they stand in memory
    const float qA = sums[0] + smooth, qB = sums[1] + smooth, qC = sums[2] + smooth, qD = sums[3] + smooth;
    const float Tp = qA / qB, Ts = qC / qD;
    const float den = (Tp + Ts) * (Tp + Ts);
    const float dTp = 2.f * Ts * Ts / den, dTs = 2.f * Tp * Tp / den;
    const float g1 = -scale * dTp * (qB - qA) / (qB * qB);   // G of a counted pixel with y = 1
    const float g0 = scale * dTp * qA / (qB * qB);           // ... with y = 0
    const float cd = -scale * dTs / qD;                      // the direct part's factor of skel(y)
    for (int lr = ty; lr < RW; lr += 8) {
        const int gr = r0 + lr;
        for (int lc = tx; lc < RW; lc += 32) {
            const int gc = c0 + lc, li = lr * RW + lc;
            float G = 0.f;
            if (gr >= 0 && gr < H && gc >= 0 && gc < W) {
                const int64_t lab = labels[img + (long)gr * W + gc];
                G = lab == 1 ? g1 : (lab == 0 ? g0 : 0.f);
            }
            gS[li] = G;
            bufs[0][li] = bufs[1][li] = bufs[2][li] = 0.f;
            code[li] = 0;
        }
    }
    int ia = 0, ig = 1, in = 2;   // a_j (becomes gE_j in place), gE_{j+1}, a_{j-1}
    __syncthreads();
    for (int j = k + 1; j >= 0; --j) {
        float* bA = bufs[ia];
        const float* bG = bufs[ig];
        float* bN = bufs[in];
        const float* Ej = j == 0 ? prob : maps + (long)(j - 1) * N;
        {   // E_j on the tile +- (j + 2)
            const int lo = hh - (j + 2), hi = RW - lo;
            for (int lr = lo + ty; lr < hi; lr += 8) {
                const int gr = r0 + lr;
                for (int lc = lo + tx; lc < hi; lc += 32) {
                    const int gc = c0 + lc;
                    Eb[lr * RW + lc] = (gr >= 0 && gr < H && gc >= 0 && gc < W) ? Ej[img + (long)gr * W + gc] : 0.f;
                }
            }
        }
        __syncthreads();
        {   // the winners of both windows of E_j, and a_{j-1}, on the tile +- (j + 1)
            const int lo = hh - (j + 1), hi = RW - lo;
            const float* Ep = j <= 1 ? prob : maps + (long)(j - 2) * N;             // E_{j-1}
            const float* Sq = j >= 2 ? maps + (long)(k + 1 + (j - 2)) * N : prob;   // S_{j-2} (not read below j = 2)
            for (int lr = lo + ty; lr < hi; lr += 8) {
                const int gr = r0 + lr;
                if (gr < 0 || gr >= H) continue;
                for (int lc = lo + tx; lc < hi; lc += 32) {
                    const int gc = c0 + lc;
                    if (gc < 0 || gc >= W) continue;
                    const int li = lr * RW + lc;
                    const float* e = Eb + li;
                    float vm = 0.f, vx = 0.f;
                    int cm = -1, cx = -1;
                    CL_MIN(gr > 0, e[-RW], 0)
                    CL_MIN(gc > 0, e[-1], 1)
                    CL_MIN(true, e[0], 2)
                    CL_MIN(gc < W - 1, e[1], 3)
                    CL_MIN(gr < H - 1, e[RW], 4)
#pragma unroll
                    for (int dr = -1; dr <= 1; ++dr)
#pragma unroll
                        for (int dc = -1; dc <= 1; ++dc)
                            CL_MAX(gr + dr >= 0 && gr + dr < H && gc + dc >= 0 && gc + dc < W, e[dr * RW + dc], (dr + 1) * 3 + dc + 1)
                    code[li] = (unsigned char)(cm | (cx << 3));
                    if (j >= 1) {
                        const long g = img + (long)gr * W + gc;
                        const float df = Ep[g] - vx;                 // E_{j-1} - O_{j-1}
                        const float d = df > 0.f ? df : 0.f;
                        const float gs = gS[li];                     // d objective / d S_{j-1}
                        float gd = gs;
                        if (j >= 2) {
                            const float sp = Sq[g];
                            const float sd = sp * d;
                            const float uu = d - sd;
                            gd = uu > 0.f ? gs * (1.f - sp) : 0.f;
                            if (uu > 0.f) gS[li] = gs * (1.f - d);   // -> d objective / d S_{j-2}
                        }
                        bN[li] = df > 0.f ? gd : 0.f;
                    }
                }
            }
        }
        __syncthreads();
        {   // gE_j on the tile +- j: every pixel collects from the windows it won
            const int lo = hh - j, hi = RW - lo;
            for (int lr = lo + ty; lr < hi; lr += 8) {
                const int gr = r0 + lr;
                if (gr < 0 || gr >= H) continue;
                for (int lc = lo + tx; lc < hi; lc += 32) {
                    const int gc = c0 + lc;
                    if (gc < 0 || gc >= W) continue;
                    const int li = lr * RW + lc;
                    float g = bA[li];
                    if (gr > 0 && (code[li - RW] & 7) == 4) g += bG[li - RW];
                    if (gc > 0 && (code[li - 1] & 7) == 3) g += bG[li - 1];
                    if ((code[li] & 7) == 2) g += bG[li];
                    if (gc < W - 1 && (code[li + 1] & 7) == 1) g += bG[li + 1];
                    if (gr < H - 1 && (code[li + RW] & 7) == 0) g += bG[li + RW];
                    if (j >= 1) {
#pragma unroll
                        for (int dr = -1; dr <= 1; ++dr)
#pragma unroll
                            for (int dc = -1; dc <= 1; ++dc)
                                if (gr + dr >= 0 && gr + dr < H && gc + dc >= 0 && gc + dc < W &&
                                    (code[li + dr * RW + dc] >> 3) == (1 - dr) * 3 + (1 - dc))
                                    g -= bN[li + dr * RW + dc];
                    }
                    bA[li] = g;
                }
            }
        }
        __syncthreads();
        const int o = ia;
        ia = in;
        in = ig;
        ig = o;
    }
    // gE_0 of the tile is in bufs[ig]; ignored pixels are constants: 0
    const float* gE = bufs[ig];
    for (int tr = ty; tr < CL_BWD_TILE; tr += 8) {
        const int gr = tcy * CL_BWD_TILE + tr, gc = tcx * CL_BWD_TILE + tx;
        if (tx >= CL_BWD_TILE || gr >= H || gc >= W) continue;
        const long g = img + (long)gr * W + gc;
        const int64_t lab = labels[g];
        const float sk = cd * skel_y[g];
        gprob[g] = (lab == 0 || lab == 1) ? gE[(tr + hh) * RW + tx + hh] + sk : 0.f;
    }
}

// ---- host-side launchers
static inline int cl_cdiv(int a, int b) { return (a + b - 1) / b; }
long cl_fwd_tiles(int B, int H, int W) { return (long)B * cl_cdiv(H, CL_FWD_TILE) * cl_cdiv(W, CL_FWD_TILE); }
size_t cl_ws_floats(int B, int H, int W, int iters) {
    return (size_t)(2 * iters + 1) * ((size_t)B * H * W) + (size_t)cl_fwd_tiles(B, H, W) * 4;
}
hipError_t cl_fwd(const float* prob, const int64_t* labels, int iters, float* skel_p, float* skel_y, float* sums, float* ws, int B, int H, int W,
                  hipStream_t st) {
    const long N = (long)B * H * W;
    const int tiles_x = cl_cdiv(W, CL_FWD_TILE), tiles_y = cl_cdiv(H, CL_FWD_TILE), nb = (int)cl_fwd_tiles(B, H, W);
    float* partial = ws + (size_t)(2 * iters + 1) * N;
    hipLaunchKernelGGL(k_cldice_fwd, dim3(nb), dim3(256), 0, st, prob, labels, iters, skel_p, skel_y, ws, partial, H, W, tiles_x, tiles_y, N);
    hipLaunchKernelGGL(k_cldice_final, dim3(1), dim3(256), 0, st, partial, sums, nb);
    return hipGetLastError();
}
hipError_t cl_bwd(const float* prob, const int64_t* labels, const float* skel_y, const float* sums, int iters, float scale, float smooth,
                  float* gprob, const float* ws, int B, int H, int W, hipStream_t st) {
    const long N = (long)B * H * W;
    const int tiles_x = cl_cdiv(W, CL_BWD_TILE), tiles_y = cl_cdiv(H, CL_BWD_TILE);
    hipLaunchKernelGGL(k_cldice_bwd, dim3((unsigned)((long)B * tiles_x * tiles_y)), dim3(256), 0, st, prob, labels, skel_y, sums, ws, iters, scale,
                       smooth, gprob, H, W, tiles_x, tiles_y, N);
    return hipGetLastError();
}
