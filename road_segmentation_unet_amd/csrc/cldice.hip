#include "cldice.h"

#include "head_stages.h"

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

// ---- the training head that takes d objective / d prob (rsu_head_fwd_bwd_aux): k_head_focal<DICE> (loss.hip) and, with FOCAL == false, the
// cross-entropy lines of k_head_loss<DICE> (elementwise.hip), with one more line: through p1 = softmax(z)[1], d p1 / d z1 = p0 p1 = -d p1 / d z0,
// a counted pixel's gprob reaches its logits in front of dact, dw and db. An ignored pixel's gprob is never loaded. loss_sum and weight_sum stay
// the cross-entropy part; grid, pixel-to-thread mapping, load batching, block reduce and the 2 C + 4 partials are the family's, so
// k_head_final_loss finishes it. gprob is loaded where it is used, not with the batch: the batch's registers are the family's.
// The cross-entropy instantiations keep two independent dlogits where the focal ones keep +-g: at 4 waves per SIMD (128 VGPRs) they spilled
// 4 and 8 registers to scratch, so they ask for 3 (the kernel is HBM-bound); the focal ones fit 128 as k_head_focal does.
static __device__ __forceinline__ void head_focal_aux(bool lab, float l0, float l1, float m, float s, float p0, float p1, float gamma, float& fce,
                                                      float& fg) {
#pragma clang fp contract(off)
    const float pt = lab ? p1 : p0, po = lab ? p0 : p1;
    const float ce = -((lab ? l1 : l0) - m - logf(s));
    const float F = exp2f(gamma * log2f(po));
    fce = F * ce;
    fg = F * fmaf(gamma * pt, ce, po);
}
template <bool FOCAL, bool DICE>
__global__ void __launch_bounds__(256, FOCAL ? 4 : 3) k_head_aux(const bf16_t* __restrict__ act, const float* __restrict__ w, const float* __restrict__ b,
                                                  const int64_t* __restrict__ labels, const float* __restrict__ class_w,
                                                  const float* __restrict__ pixel_w, float gamma, const float* __restrict__ dice_sums,
                                                  float dice_scale, float smooth, const float* __restrict__ gprob, float* __restrict__ prob,
                                                  bf16_t* __restrict__ dact, float* __restrict__ partial, long npix, int C, float inv_count) {
    const int LP = C >> 3;
    const int sub = threadIdx.x % LP;
    const int ppb = 256 / LP;  // pixels per block iteration
    float w0[8], w1[8], b0, b1;
    head_setup(w, b, sub, w0, w1, b0, b1);
    const float cw0 = class_w ? class_w[0] : 1.f, cw1 = class_w ? class_w[1] : 1.f;
    float gq0 = 0.f, gq1 = 0.f;
    if constexpr (DICE) {   // k_head_loss<true>'s two uniform factors
        const float dU = dice_sums[1] + dice_sums[2] + smooth;
        const float dD = (2.f * dice_sums[0] + smooth) / dU;
        gq0 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(dice_scale * dD / dU)));
        gq1 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(dice_scale * (dD - 2.f) / dU)));
    }
    float gw0[8], gw1[8], gb0 = 0.f, gb1 = 0.f, lsum = 0.f, osum = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) gw0[i] = gw1[i] = 0.f;
    const int niter = (int)((npix + (long)gridDim.x * ppb - 1) / ((long)gridDim.x * ppb));
    for (int it0 = 0; it0 < niter; it0 += HEAD_HU) {
        long pp[HEAD_HU];
        bool okk[HEAD_HU];
        u32x4 raw[HEAD_HU];
        int64_t labv[HEAD_HU];
        float pwv[HEAD_HU];
        head_load<int>(act, labels, pixel_w, it0, niter, npix, C, LP, sub, ppb, pp, okk, raw, labv, pwv);
#pragma unroll
        for (int u = 0; u < HEAD_HU; ++u) {
            const long p = pp[u];
            const bool ok = okk[u];
            float a[8], l0, l1, m, s, p0, p1;
            head_softmax(raw[u], w0, w1, b0, b1, LP, a, l0, l1, m, s, p0, p1);
            if (ok && sub == 0) prob[p] = p1;
            if (!ok) continue;
            const int64_t lab = labv[u];
            if (lab != 0 && lab != 1) {   // ignored
                *(u32x4*)(dact + p * C + sub * 8) = u32x4{0u, 0u, 0u, 0u};
                continue;
            }
            const float ga = gprob[p] * (p0 * p1);
            const float omega = (lab ? cw1 : cw0) * pwv[u];
            float d0, d1, fce = 0.f;
            if constexpr (FOCAL) {
                float fg;
                head_focal_aux(lab != 0, l0, l1, m, s, p0, p1, gamma, fce, fg);
                const float g = (omega * inv_count) * fg;
                d0 = lab ? g : -g;
                d1 = lab ? -g : g;
            } else {
                d0 = (p0 - (lab == 0 ? 1.f : 0.f)) * inv_count * omega;
                d1 = (p1 - (lab == 1 ? 1.f : 0.f)) * inv_count * omega;
                fce = -((lab ? l1 : l0) - m - logf(s));   // (formed here: l0, l1, m and s need not live through the pixel's backward)
            }
            if constexpr (DICE) {
                const float gt = pwv[u] * (p0 * p1);
                if constexpr (FOCAL) {
                    // k_head_focal<true> compiles its `d0 -= gd; d1 += gd` into one fused multiply-add each; behind the lines below the
                    // compiler rounded the product first. Written out, so that a zero gprob leaves that kernel's numbers
                    const float gq = lab ? gq1 : gq0;
                    d0 = fmaf(-gt, gq, d0);
                    d1 = fmaf(gt, gq, d1);
                } else {
                    const float gd = lab ? gt * gq1 : gt * gq0;
                    d0 -= gd;
                    d1 += gd;
                }
            }
            d0 -= ga;
            d1 += ga;
            // the pixel's backward: weight gradients, and dact through the ReLU in front of the head
            float da[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                gw0[i] = fmaf(a[i], d0, gw0[i]);
                gw1[i] = fmaf(a[i], d1, gw1[i]);
                da[i] = a[i] > 0.f ? fmaf(d0, w0[i], d1 * w1[i]) : 0.f;
            }
            *(u32x4*)(dact + p * C + sub * 8) = pack8(da);
            if (sub == 0) {
                if constexpr (FOCAL) {
#pragma clang fp contract(off)
                    gb0 += d0;
                    gb1 += d1;
                    lsum = fmaf(fce, omega, lsum);
                    osum += omega;
                } else {
                    gb0 += d0;
                    gb1 += d1;
                    lsum += omega * fce;
                    osum += omega;
                }
            }
        }
    }
    constexpr int NV = 21;
    __shared__ float red[256 * NV];
    float* my = red + threadIdx.x * NV;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        my[i] = gw0[i];
        my[8 + i] = gw1[i];
    }
    my[16] = gb0; my[17] = gb1; my[18] = lsum; my[19] = osum;
    __syncthreads();
    const int nout = 2 * C + 4;  // [C][2] dw, db[2], loss, weight sum
    for (int o = threadIdx.x; o < nout; o += 256) {
        const int c = o >> 1;
        partial[(long)blockIdx.x * nout + o] = o < 2 * C ? head_block_sum<NV>(red, c >> 3, (o & 1) * 8 + (c & 7), ppb, LP)
                                                         : head_block_sum<NV>(red, 0, 16 + (o - 2 * C), ppb, LP);
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
hipError_t cl_head_aux(const void* act, const float* w, const float* b, const int64_t* labels, const float* class_w, const float* pixel_w,
                       float gamma, const float* dice_sums, float dice_scale, float smooth, const float* gprob, float* prob, void* dact, float* dw,
                       float* db, float* loss_sum, float* weight_sum, float* ws, long npix, int C, float inv_count, hipStream_t st) {
    const int nb = ew_head_blocks(npix, C);
    auto kern = gamma > 0.f ? (dice_sums ? k_head_aux<true, true> : k_head_aux<true, false>)
                            : (dice_sums ? k_head_aux<false, true> : k_head_aux<false, false>);
    hipLaunchKernelGGL(kern, dim3(nb), dim3(256), 0, st, (const bf16_t*)act, w, b, labels, class_w, pixel_w, gamma, dice_sums, dice_scale, smooth,
                       gprob, prob, (bf16_t*)dact, ws, npix, C, inv_count);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : ew_head_final_loss(ws, dw, db, loss_sum, weight_sum, nb, C, st);
}
