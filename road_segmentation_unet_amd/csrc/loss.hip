#include "loss.h"

#include "head_stages.h"

// The focal members of the opt-in head family (include/rsu_loss.h), built from the family's stages in head_stages.h: the cross-entropy
// of a counted pixel modulated by how wrong the net is on it,
//   t = label, o = 1 - t;  F = p_o^gamma = exp2(gamma log2 p_o)  ((1 - p_t)^gamma without the cancellation);  CE = -(l_t - m - log s)
//   loss_p = omega F CE;   g = omega inv_count F (p_o + gamma p_t CE);   dlogit[t] = -g, dlogit[o] = +g
// (d/dz_t [-p_o^gamma log p_t] = p_o^gamma (gamma p_t log p_t - p_o): no division). Finite in every corner: p_o == 0 gives
// gamma * -inf = -inf, exp2(-inf) = 0, g = 0; p_t == 0 leaves CE finite (log-sum-exp form), p_t CE = 0, F = 1. gamma == 0 with p_o == 0
// would be 0 * -inf = NaN: the host never launches these kernels with gamma == 0 (rsu_api.hip takes the siblings then).
// They are a translation unit of their own so that elementwise.hip's kernels keep the ISA they shipped with (inside that file they
// changed 29 lines of k_head_sums<true>).
// One function for both kernels, nothing in it contracted: F CE (-> loss_sum with an explicit fused multiply-add behind omega) and
// F (p_o + gamma p_t CE) have the same bits in the training and in the evaluation head. log2f / exp2f are the accurate library forms
// (denormal p_o included); the kernels are HBM-bound and the sub == 0 lanes alone need the loss. gamma is a kernel argument: uniform, it
// stays in a scalar register.
static __device__ __forceinline__ void head_focal(bool lab, float l0, float l1, float m, float s, float p0, float p1, float gamma, float& fce,
                                                  float& fg) {
#pragma clang fp contract(off)
    const float pt = lab ? p1 : p0, po = lab ? p0 : p1;
    const float ce = -((lab ? l1 : l0) - m - logf(s));
    const float F = exp2f(gamma * log2f(po));
    fce = F * ce;
    fg = F * fmaf(gamma * pt, ce, po);
}
// k_head_loss<DICE> with the rule above in place of its d0 / d1 and lsum lines: same grid, pixel-to-thread mapping, load batching,
// ignored-pixel selection (+0 dact row, nothing summed), Dice term (added to dlogit as there; neither the class weights nor F enter it),
// LDS block reduce and 2 C + 4 partial layout, so k_head_final_loss finishes it. weight_sum stays sum omega (k_head_loss's bits).
// Both instantiations take the 32-bit trip count. Registers and occupancy: profiles/r18/focal.txt.
template <bool DICE>
__global__ void __launch_bounds__(256, 4) k_head_focal(const bf16_t* __restrict__ act, const float* __restrict__ w, const float* __restrict__ b,
                                                    const int64_t* __restrict__ labels, const float* __restrict__ class_w,
                                                    const float* __restrict__ pixel_w, float gamma, const float* __restrict__ dice_sums,
                                                    float dice_scale, float smooth, float* __restrict__ prob, bf16_t* __restrict__ dact,
                                                    float* __restrict__ partial, long npix, int C, float inv_count) {
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
            const float omega = (lab ? cw1 : cw0) * pwv[u];
            float fce, fg;
            head_focal(lab != 0, l0, l1, m, s, p0, p1, gamma, fce, fg);
            const float g = (omega * inv_count) * fg;
            float d0 = lab ? g : -g;
            float d1 = lab ? -g : g;
            if constexpr (DICE) {
                const float gt = pwv[u] * (p0 * p1);
                const float gd = lab ? gt * gq1 : gt * gq0;
                d0 -= gd;
                d1 += gd;
            }
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
#pragma clang fp contract(off)
                gb0 += d0;
                gb1 += d1;
                lsum = fmaf(fce, omega, lsum);
                osum += omega;
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
// k_head_sums<true> with omega F CE in the first sum: sum omega, {I, P, Y} and the LDS histogram with its per-block rows are its
// expressions in its order (the same bits), and k_head_eval_final finishes it.
__global__ void __launch_bounds__(256, 4) k_head_sums_focal(const bf16_t* __restrict__ act, const float* __restrict__ w, const float* __restrict__ b,
                                                         const int64_t* __restrict__ labels, const float* __restrict__ class_w,
                                                         const float* __restrict__ pixel_w, float gamma, float* __restrict__ prob,
                                                         float* __restrict__ partial, unsigned* __restrict__ hpart, long npix, int C) {
    constexpr int NS = 5;
    const int LP = C >> 3;
    const int sub = threadIdx.x % LP;
    const int ppb = 256 / LP;  // pixels per block iteration
    __shared__ unsigned hist[2 * EW_EVAL_BINS];
    for (int i = threadIdx.x; i < 2 * EW_EVAL_BINS; i += 256) hist[i] = 0u;
    float w0[8], w1[8], b0, b1;
    head_setup(w, b, sub, w0, w1, b0, b1);
    const float cw0 = class_w ? class_w[0] : 1.f, cw1 = class_w ? class_w[1] : 1.f;
    float lsum = 0.f, osum = 0.f, si = 0.f, sp = 0.f, sy = 0.f;
    __syncthreads();
    const long niter = (npix + (long)gridDim.x * ppb - 1) / ((long)gridDim.x * ppb);
    for (long it0 = 0; it0 < niter; it0 += HEAD_HU) {
        long pp[HEAD_HU];
        bool okk[HEAD_HU];
        u32x4 raw[HEAD_HU];
        int64_t labv[HEAD_HU];
        float pwv[HEAD_HU];
        head_load<long>(act, labels, pixel_w, it0, niter, npix, C, LP, sub, ppb, pp, okk, raw, labv, pwv);
#pragma unroll
        for (int u = 0; u < HEAD_HU; ++u) {
            float a[8], l0, l1, m, s, p0, p1;
            head_softmax(raw[u], w0, w1, b0, b1, LP, a, l0, l1, m, s, p0, p1);
            if (!okk[u] || sub != 0) continue;
            prob[pp[u]] = p1;
            const int64_t lab = labv[u];
            if (lab != 0 && lab != 1) continue;   // ignored: no loss, no weight, no mass, no count, whatever its pixel_w holds
            {
#pragma clang fp contract(off)
                const float omega = (lab ? cw1 : cw0) * pwv[u];
                float fce, fg;
                head_focal(lab != 0, l0, l1, m, s, p0, p1, gamma, fce, fg);
                lsum = fmaf(fce, omega, lsum);
                osum += omega;
                sp = fmaf(pwv[u], p1, sp);
                if (lab) {
                    si = fmaf(pwv[u], p1, si);
                    sy += pwv[u];
                }
            }
            const int bin = max(0, min(EW_EVAL_BINS - 1, (int)(p1 * (float)EW_EVAL_BINS)));
            atomicAdd(&hist[(int)lab * EW_EVAL_BINS + bin], 1u);
        }
    }
    // block reduce: the threads with sub == 0 hold the sums
    __shared__ float red[256 * NS];
    float* my = red + threadIdx.x * NS;
    my[0] = lsum;
    my[1] = osum;
    my[2] = si;
    my[3] = sp;
    my[4] = sy;
    __syncthreads();
    if (threadIdx.x < NS) partial[(long)blockIdx.x * NS + threadIdx.x] = head_block_sum<NS>(red, 0, threadIdx.x, ppb, LP);
    for (int i = threadIdx.x; i < 2 * EW_EVAL_BINS; i += 256) hpart[(long)blockIdx.x * (2 * EW_EVAL_BINS) + i] = hist[i];
}

// the focal heads (gamma > 0: the caller sends gamma == 0 to ew_head_loss / ew_head_eval): the grids, workspaces and final kernels of those
hipError_t ew_head_focal(const void* act, const float* w, const float* b, const int64_t* labels, const float* class_w, const float* pixel_w,
                         float gamma, const float* dice_sums, float dice_scale, float smooth, float* prob, void* dact, float* dw, float* db,
                         float* loss_sum, float* weight_sum, float* ws, long npix, int C, float inv_count, hipStream_t st) {
    const int nb = ew_head_blocks(npix, C);
    hipLaunchKernelGGL(dice_sums ? k_head_focal<true> : k_head_focal<false>, dim3(nb), dim3(256), 0, st, (const bf16_t*)act, w, b, labels, class_w,
                       pixel_w, gamma, dice_sums, dice_scale, smooth, prob, (bf16_t*)dact, ws, npix, C, inv_count);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : ew_head_final_loss(ws, dw, db, loss_sum, weight_sum, nb, C, st);
}
hipError_t ew_head_eval_focal(const void* act, const float* w, const float* b, const int64_t* labels, const float* class_w, const float* pixel_w,
                              float gamma, float* prob, float* sums, unsigned long long* hist, float* ws, long npix, int C, hipStream_t st) {
    const int nb = ew_head_blocks(npix, C);
    unsigned* hpart = (unsigned*)(ws + (size_t)nb * 5);   // ew_head_eval's layout
    hipLaunchKernelGGL(k_head_sums_focal, dim3(nb), dim3(256), 0, st, (const bf16_t*)act, w, b, labels, class_w, pixel_w, gamma, prob, ws, hpart, npix,
                       C);
    const hipError_t e = hipGetLastError();
    return e != hipSuccess ? e : ew_head_eval_final(ws, hpart, sums, hist, nb, st);
}
