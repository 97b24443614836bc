// The head: 1x1 conv (C -> 2) + softmax[..., 1], with the loss and its backward fused in. HBM-bound: one 16-byte (8 x bf16) access per lane,
// LP = C / 8 lanes per pixel, partial logits met with wave shuffles.
// Two sets of kernels. k_head<TRAIN> and k_head_final are PINNED: the unweighted step is on the critical queue, and sharing k_head's body
// through an inlined function template moved its register allocation (1500 of 1585 ISA lines), so they are written out and nothing below
// is shared with them. Every opt-in head is one of two templates built from the head_* stages below: k_head_train<FOCAL, DICE, AUX>
// (forward, loss and backward; k_head_final_loss finishes it) and the forward-only k_head_sums<EVAL, FOCAL> (k_head_final_dice_sums or
// k_head_eval_final finishes it). Their grid, pixel-to-thread mapping and the order of every sum are k_head<true>'s.
#include "head.h"

// ---------------------------------------------------------------------------------------------
// the pinned pair
// ---------------------------------------------------------------------------------------------
template <bool TRAIN>
__global__ void __launch_bounds__(256) k_head(const bf16_t* __restrict__ act, const float* __restrict__ w, const float* __restrict__ b,
                                              const int64_t* __restrict__ labels, float* __restrict__ prob, float* __restrict__ logits,
                                              bf16_t* __restrict__ dact, float* __restrict__ partial, long npix, int C, float inv_count) {
    const int LP = C >> 3;
    const int sub = threadIdx.x % LP;
    const int ppb = 256 / LP;  // pixels per block iteration
    float w0[8], w1[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        w0[i] = w[(sub * 8 + i) * 2];
        w1[i] = w[(sub * 8 + i) * 2 + 1];
    }
    const float b0 = b[0], b1 = b[1];
    float gw0[8], gw1[8], gb0 = 0.f, gb1 = 0.f, lsum = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) gw0[i] = gw1[i] = 0.f;
    const long niter = (npix + (long)gridDim.x * ppb - 1) / ((long)gridDim.x * ppb);
    // HU pixels per thread and trip, all loads requested before any is used: the HBM latency (~2 us x 6 TB/s = 47 KB per CU in flight) wants more
    // than the 16-32 KB that one or two 16-byte loads per lane of 16-20 resident waves give (round 5: two, 3.87 TB/s; round 6: four). The sums keep
    // the order of the pixels: same bits.
    constexpr int HU = 4;
    for (long it0 = 0; it0 < niter; it0 += HU) {
        long pp[HU];
        bool okk[HU];
        u32x4 raw[HU];
        int labv[HU];
#pragma unroll
        for (int u = 0; u < HU; ++u) {
            labv[u] = 0;
            pp[u] = ((it0 + u) * gridDim.x + blockIdx.x) * ppb + threadIdx.x / LP;
            okk[u] = (it0 + u < niter) && pp[u] < npix;
            raw[u] = okk[u] ? *(const u32x4*)(act + pp[u] * C + sub * 8) : u32x4{0u, 0u, 0u, 0u};
            if (TRAIN) labv[u] = okk[u] ? (int)labels[pp[u]] : 0;
        }
#pragma unroll
        for (int u = 0; u < HU; ++u) {
            const long p = pp[u];
            const bool ok = okk[u];
            float a[8];
            unpack8(raw[u], a);
            float l0 = 0.f, l1 = 0.f;
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
            const float m = fmaxf(l0, l1);
            const float e0 = expf(l0 - m), e1 = expf(l1 - m);
            const float s = e0 + e1;
            const float p1 = e1 / s, p0 = e0 / s;
            if (ok && sub == 0) {
                prob[p] = p1;
                if (logits) {
                    logits[2 * p] = l0;
                    logits[2 * p + 1] = l1;
                }
            }
            if (TRAIN) {
                if (ok) {
                    const int lab = labv[u];
                    const float d0 = (p0 - (lab == 0 ? 1.f : 0.f)) * inv_count;
                    const float d1 = (p1 - (lab == 1 ? 1.f : 0.f)) * inv_count;
                    float da[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        gw0[i] = fmaf(a[i], d0, gw0[i]);
                        gw1[i] = fmaf(a[i], d1, gw1[i]);
                        da[i] = a[i] > 0.f ? fmaf(d0, w0[i], d1 * w1[i]) : 0.f;
                    }
                    *(u32x4*)(dact + p * C + sub * 8) = pack8(da);
                    if (sub == 0) {
                        gb0 += d0;
                        gb1 += d1;
                        lsum += -((lab ? l1 : l0) - m - logf(s));
                    }
                }
            }
        }
    }
    if (TRAIN) {
        // block reduce: threads with equal `sub` hold partials for the same 8 channels
        __shared__ float red[256 * 19];
        float* my = red + threadIdx.x * 19;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            my[i] = gw0[i];
            my[8 + i] = gw1[i];
        }
        my[16] = gb0; my[17] = gb1; my[18] = lsum;
        __syncthreads();
        const int nout = 2 * C + 3;  // [C][2] dw, db[2], loss
        for (int o = threadIdx.x; o < nout; o += 256) {
            float t = 0.f;
            if (o < 2 * C) {
                const int c = o >> 1, k = o & 1, sg = c >> 3, i = c & 7;
                for (int q = 0; q < ppb; ++q) t += red[(q * LP + sg) * 19 + k * 8 + i];
            } else {
                const int j = 16 + (o - 2 * C);
                for (int q = 0; q < ppb; ++q) t += red[(q * LP) * 19 + j];
            }
            partial[(long)blockIdx.x * nout + o] = t;
        }
    }
}
template __global__ void k_head<true>(const bf16_t*, const float*, const float*, const int64_t*, float*, float*, bf16_t*, float*, long, int, float);
template __global__ void k_head<false>(const bf16_t*, const float*, const float*, const int64_t*, float*, float*, bf16_t*, float*, long, int, float);

__global__ void __launch_bounds__(256) k_head_final(const float* __restrict__ partial, float* __restrict__ dw, float* __restrict__ db,
                                                    float* __restrict__ loss_sum, int nblk, int C) {
    // one wave per output (four per workgroup): lane l sums partials l, l + 64, ... (independent loads), then a fixed-order butterfly;
    // 2 C + 3 outputs of ~1000 partials each -- with 32 lanes per output in 17 workgroups the kernel was a chain of ~32 dependent
    // L2 round trips (11 us)
    const int nout = 2 * C + 3;
    const int o = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (o >= nout) return;
    float t = 0.f;
    for (int bk = lane; bk < nblk; bk += 64) t += partial[(long)bk * nout + o];
    for (int m = 32; m > 0; m >>= 1) t += __shfl_xor(t, m);
    if (lane == 0) {
        if (o < 2 * C) dw[o] = t;
        else if (o < 2 * C + 2) db[o - 2 * C] = t;
        else loss_sum[0] += t;
    }
}

// ---------------------------------------------------------------------------------------------
// the opt-in family: its stages
// ---------------------------------------------------------------------------------------------
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
// HU pixels per thread and trip as in k_head; the pixel's 64-bit label and its weight are requested with its activations, before any is used.
// The trip count is an int: at most 8 below 1024 blocks and npix / (1024 ppb) above, where npix C 2 bytes < 2 GiB (rsu_api.hip refuses more).
constexpr int HEAD_HU = 4;
static __device__ __forceinline__ int head_trips(long npix, int ppb) { return (int)((npix + (long)gridDim.x * ppb - 1) / ((long)gridDim.x * ppb)); }
static __device__ __forceinline__ void head_load(const bf16_t* __restrict__ act, const int64_t* __restrict__ labels, const float* __restrict__ pixel_w,
                                                 int it0, int niter, long npix, int C, int LP, int sub, int ppb, long (&pp)[HEAD_HU],
                                                 bool (&okk)[HEAD_HU], u32x4 (&raw)[HEAD_HU], int64_t (&labv)[HEAD_HU], float (&pwv)[HEAD_HU]) {
#pragma unroll
    for (int u = 0; u < HEAD_HU; ++u) {
        pp[u] = ((long)(it0 + u) * gridDim.x + blockIdx.x) * ppb + threadIdx.x / LP;
        okk[u] = (it0 + u < niter) && pp[u] < npix;
        raw[u] = okk[u] ? *(const u32x4*)(act + pp[u] * C + sub * 8) : u32x4{0u, 0u, 0u, 0u};
        labv[u] = okk[u] ? labels[pp[u]] : 0;
        pwv[u] = (okk[u] && pixel_w) ? pixel_w[pp[u]] : 1.f;
    }
    // The batch's last load is waited for here, in front of the trip's first store. Loads and stores share one counter: a wait for this value
    // further down, behind a store, is a wait for that store's round trip as well (2.8 us of 47 per call at npix = 4 x 388 x 388, C = 64: profiles/r24/head_fold.txt).
    asm volatile("" : "+v"(pwv[HEAD_HU - 1]));
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
// the cross-entropy of a counted pixel, CE = -(l_t - m - log s), in k_head's expression
static __device__ __forceinline__ float head_ce(bool lab, float l0, float l1, float m, float s) { return -((lab ? l1 : l0) - m - logf(s)); }
// The focal rule (include/rsu_loss.h): the cross-entropy of a counted pixel modulated by how wrong the net is on it,
//   t = label, o = 1 - t;  F = p_o^gamma = exp2(gamma log2 p_o)  ((1 - p_t)^gamma without the cancellation);  CE as above
//   loss_p = omega F CE;   g = omega inv_count F (p_o + gamma p_t CE);   dlogit[t] = -g, dlogit[o] = +g
// (d/dz_t [-p_o^gamma log p_t] = p_o^gamma (gamma p_t log p_t - p_o): no division). Finite in every corner: p_o == 0 gives
// gamma * -inf = -inf, exp2(-inf) = 0, g = 0; p_t == 0 leaves CE finite (log-sum-exp form), p_t CE = 0, F = 1. gamma == 0 with p_o == 0
// would be 0 * -inf = NaN: the host never launches a FOCAL instantiation with gamma == 0 (hd_train and hd_eval take the others then).
// Returns fce = F CE and fg = F (p_o + gamma p_t CE), nothing contracted: the same bits in the training and in the evaluation head.
// log2f / exp2f are the accurate library forms (denormal p_o included); the kernels are HBM-bound and the sub == 0 lanes alone need the
// loss. gamma is a kernel argument: uniform, it stays in a scalar register.
static __device__ __forceinline__ void head_focal(bool lab, float l0, float l1, float m, float s, float p0, float p1, float gamma, float& fce,
                                                  float& fg) {
#pragma clang fp contract(off)
    const float pt = lab ? p1 : p0, po = lab ? p0 : p1;
    const float ce = head_ce(lab, l0, l1, m, s);
    const float F = exp2f(gamma * log2f(po));
    fce = F * ce;
    fg = F * fmaf(gamma * pt, ce, po);
}
// block reduce over rows of NV floats, one row per thread (an odd NV keeps the rows on different LDS banks): value j of the threads that
// hold channel group sg, in the order of their pixels
template <int NV>
static __device__ __forceinline__ float head_block_sum(const float* red, int sg, int j, int ppb, int LP) {
    float t = 0.f;
    for (int q = 0; q < ppb; ++q) t += red[(q * LP + sg) * NV + j];
    return t;
}

// ---------------------------------------------------------------------------------------------
// the training heads
// ---------------------------------------------------------------------------------------------
// k_head<true> with omega = class_w[label] * pixel_w[pixel] in front of the pixel's loss and dlogits. A label that is neither 0 nor 1
// (tested on all 64 bits) means omega = 0 BY SELECTION, never by multiplication: the pixel's dact row is stored as +0 and it is left out of
// every sum, whatever its pixel_w (or gprob) holds. One more per-thread sum (omega -> weight_sum) rides through the block reduce: 2 C + 4
// partials per block. x * 1.0f is exact: with every omega == 1, <false, false, false> has k_head<true>'s bits.
// The terms, each in front of the weight / bias gradients and dact; loss_sum and weight_sum stay the (focal) cross-entropy part:
//   FOCAL  the rule of head_focal in place of the plain cross-entropy's dlogits and loss;
//   DICE   (pass B of the soft-Dice head) the gradient of dice_scale * (1 - D),
//            gd = dice_scale * m (D - 2 y) / U * p0 p1   added to dlogit 1 and taken from dlogit 0,   U = P + Y + smooth, D = (2 I + smooth) / U,
//          m the pixel's pixel_w; neither the class weights nor F enter it. {I, P, Y} are READ from dice_sums (three uniform loads per
//          thread; what pass A left there, or what a host made of it);
//   AUX    a given d objective / d prob: through p1 = softmax(z)[1], d p1 / d z1 = p0 p1 = -d p1 / d z0,
//            ga = gprob * p0 p1   added to dlogit 1 and taken from dlogit 0.
//          gprob is loaded where it is used, not with the batch, and never for an ignored pixel.
// Nothing in the kernel is left to the compiler to contract: where a product and a sum share one rounding, a fused multiply-add says so.
// The rule (these are the bits every instantiation has had since it shipped): the plain cross-entropy's product with omega takes the first
// further term, itself a rounded product, as its addend, and a second one is added to the result; behind the focal dlogits +-g every
// further term is one fused multiply-add of its two factors. A term that is zero leaves the bits of the instantiation without it.
// Registers: 4 waves per SIMD asked for (<= 128 VGPRs, k_head<true>'s occupancy; the 64-bit labels and the weights in flight cost 131
// without). Every instantiation fits without scratch: profiles/r24/head_fold.txt.
template <bool FOCAL, bool DICE, bool AUX>
__global__ void __launch_bounds__(256, 4)
    k_head_train(const bf16_t* __restrict__ act, const float* __restrict__ w, const float* __restrict__ b, const int64_t* __restrict__ labels,
                 const float* __restrict__ class_w, const float* __restrict__ pixel_w, float gamma, const float* __restrict__ dice_sums,
                 float dice_scale, float smooth, const float* __restrict__ gprob, float* __restrict__ prob, bf16_t* __restrict__ dact,
                 float* __restrict__ partial, long npix, int C, float inv_count) {
#pragma clang fp contract(off)
    const int LP = C >> 3;
    const int sub = threadIdx.x % LP;
    const int ppb = 256 / LP;  // pixels per block iteration
    float w0[8], w1[8], b0, b1;
    head_setup(w, b, sub, w0, w1, b0, b1);
    const float cw0 = class_w ? class_w[0] : 1.f, cw1 = class_w ? class_w[1] : 1.f;
    float gq0 = 0.f, gq1 = 0.f;
    if constexpr (DICE) {
        const float dU = dice_sums[1] + dice_sums[2] + smooth;
        const float dD = (2.f * dice_sums[0] + smooth) / dU;
        // dice_scale (D - 2 y) / U for y = 0 and y = 1: the same in every lane, so kept in scalar registers (as plain floats they cost the
        // vector registers that the kernel does not have to spare at 4 waves per SIMD)
        gq0 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(dice_scale * dD / dU)));
        gq1 = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(dice_scale * (dD - 2.f) / dU)));
    }
    float gw0[8], gw1[8], gb0 = 0.f, gb1 = 0.f, lsum = 0.f, osum = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) gw0[i] = gw1[i] = 0.f;
    const int niter = head_trips(npix, ppb);
    for (int it0 = 0; it0 < niter; it0 += HEAD_HU) {
        long pp[HEAD_HU];
        bool okk[HEAD_HU];
        u32x4 raw[HEAD_HU];
        int64_t labv[HEAD_HU];
        float pwv[HEAD_HU];
        head_load(act, labels, pixel_w, it0, niter, npix, C, LP, sub, ppb, pp, okk, raw, labv, pwv);
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
            const float pq = p0 * p1;
            float gp = 0.f, gt = 0.f, gq = 0.f;   // the further terms' factors: ga = gp pq, gd = gt gq
            if constexpr (AUX) gp = gprob[p];
            if constexpr (DICE) {
                gt = pwv[u] * pq;
                gq = lab ? gq1 : gq0;
            }
            float d0, d1, fce;
            if constexpr (FOCAL) {
                float fg;
                head_focal(lab != 0, l0, l1, m, s, p0, p1, gamma, fce, fg);
                const float g = (omega * inv_count) * fg;
                d0 = lab ? g : -g;
                d1 = lab ? -g : g;
                if constexpr (DICE) {
                    d0 = fmaf(-gt, gq, d0);
                    d1 = fmaf(gt, gq, d1);
                }
                if constexpr (AUX) {
                    d0 = fmaf(-gp, pq, d0);
                    d1 = fmaf(gp, pq, d1);
                }
            } else {
                fce = head_ce(lab != 0, l0, l1, m, s);
                const float t0 = (p0 - (lab == 0 ? 1.f : 0.f)) * inv_count;
                const float t1 = (p1 - (lab == 1 ? 1.f : 0.f)) * inv_count;
                if constexpr (DICE || AUX) {
                    const float g = DICE ? gt * gq : gp * pq;
                    d0 = fmaf(t0, omega, -g);
                    d1 = fmaf(t1, omega, g);
                    if constexpr (DICE && AUX) {
                        const float ga = gp * pq;
                        d0 -= ga;
                        d1 += ga;
                    }
                } else {
                    d0 = t0 * omega;
                    d1 = t1 * omega;
                }
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
                gb0 += d0;
                gb1 += d1;
                lsum = fmaf(fce, omega, lsum);
                osum += omega;
            }
        }
    }
    // block reduce as in k_head, one more value per thread: threads with equal `sub` hold partials for the same 8 channels
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
// k_head_final over 2 C + 4 outputs: the last one is the sum of the weights (weight_sum may be NULL: not wanted). Same lanes, same order.
__global__ void __launch_bounds__(256) k_head_final_loss(const float* __restrict__ partial, float* __restrict__ dw, float* __restrict__ db,
                                                         float* __restrict__ loss_sum, float* __restrict__ weight_sum, int nblk, int C) {
    const int nout = 2 * C + 4;
    const int o = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (o >= nout) return;
    const float t = head_final_sum(partial, nblk, nout, o, lane);
    if (lane == 0) {
        if (o < 2 * C) dw[o] = t;
        else if (o < 2 * C + 2) db[o - 2 * C] = t;
        else if (o == 2 * C + 2) loss_sum[0] += t;
        else if (weight_sum) weight_sum[0] += t;
    }
}

// ---------------------------------------------------------------------------------------------
// the forward-only heads
// ---------------------------------------------------------------------------------------------
// k_head_train's grid, pixel-to-thread mapping, load batching and logit / softmax expressions (prob gets the same bits); no dact, no dw, no
// db. Per thread (the sub == 0 lane of a pixel) the sums
//   I = sum m p y, P = sum m p, Y = sum m y   with the pixel's mass m = pixel_w (1 without a map),
// and with EVAL in front of them {omega CE, omega} -- with FOCAL {omega F CE, omega} -- in k_head_train's expressions and order: the bits
// of the training head's loss_sum and weight_sum. Everything 0 BY SELECTION for a label that is neither 0 nor 1 (all 64 bits). NS = 3 or 5
// partials per block, in the order of k_head_train's scalar outputs.
// <false, false> (rsu_head_dice_sums) is pass A of the soft-Dice head: the Dice gradient of a pixel needs {I, P, Y} over the whole batch,
// so the head runs twice. class_w, gamma and hpart are not touched. (<false, true> does not exist: pass A has no loss.)
// <true, *> (rsu_head_eval, rsu_head_eval_focal) is the evaluation head for held-out data: it also keeps, for every counted pixel, one
// count in the block's LDS histogram hist[label][min(255, (int)(p * 256))].
// The histogram: one LDS counter array per block (2 x 256 u32), bumped by the pixel's sub == 0 lane only -- at most 64 / LP lanes of a
// wave, so a trained network that sends every pixel to bin 0 or bin 255 costs a wave at most that many serialised LDS adds per pixel
// trip, next to 64 16-byte HBM loads. Blocks never meet on a global address: each stores its 512 counters as a plain row of the
// workspace (2 KB per block, 2 MB at 1024 blocks against 77 MB of activations read), and k_head_eval_final sums the rows. 1024 blocks
// adding to the two hot addresses of a saturated histogram at the same moment is exactly what this avoids.
template <bool EVAL, bool FOCAL>
__global__ void __launch_bounds__(256, 4) k_head_sums(const bf16_t* __restrict__ act, const float* __restrict__ w, const float* __restrict__ b,
                                                   const int64_t* __restrict__ labels, const float* __restrict__ class_w,
                                                   const float* __restrict__ pixel_w, float gamma, float* __restrict__ prob,
                                                   float* __restrict__ partial, unsigned* __restrict__ hpart, long npix, int C) {
    static_assert(EVAL || !FOCAL, "pass A of the soft-Dice head has no loss to modulate");
    constexpr int NS = EVAL ? 5 : 3;
    const int LP = C >> 3;
    const int sub = threadIdx.x % LP;
    const int ppb = 256 / LP;  // pixels per block iteration
    __shared__ unsigned hist[EVAL ? 2 * EW_EVAL_BINS : 1];   // (<false, false> never names it: no LDS is set aside)
    if constexpr (EVAL)
        for (int i = threadIdx.x; i < 2 * EW_EVAL_BINS; i += 256) hist[i] = 0u;
    float w0[8], w1[8], b0, b1;
    head_setup(w, b, sub, w0, w1, b0, b1);
    float cw0 = 1.f, cw1 = 1.f;
    if constexpr (EVAL) {
        cw0 = class_w ? class_w[0] : 1.f;
        cw1 = class_w ? class_w[1] : 1.f;
    }
    float lsum = 0.f, osum = 0.f, si = 0.f, sp = 0.f, sy = 0.f;
    if constexpr (EVAL) __syncthreads();
    const int niter = head_trips(npix, ppb);
    for (int it0 = 0; it0 < niter; it0 += HEAD_HU) {
        long pp[HEAD_HU];
        bool okk[HEAD_HU];
        u32x4 raw[HEAD_HU];
        int64_t labv[HEAD_HU];
        float pwv[HEAD_HU];
        head_load(act, labels, pixel_w, it0, niter, npix, C, LP, sub, ppb, pp, okk, raw, labv, pwv);
#pragma unroll
        for (int u = 0; u < HEAD_HU; ++u) {
            float a[8], l0, l1, m, s, p0, p1;
            head_softmax(raw[u], w0, w1, b0, b1, LP, a, l0, l1, m, s, p0, p1);
            if (!okk[u] || sub != 0) continue;
            prob[pp[u]] = p1;
            const int64_t lab = labv[u];
            if (lab != 0 && lab != 1) continue;   // ignored: no loss, no weight, no mass, no count, whatever its pixel_w holds
            {
                // nothing contracted, the fused forms written out: k_head_train's loss and weight sums, and the same {I, P, Y} from both
                // instantiations (left to the compiler, three sums side by side and five came out one ulp apart on a block's sum)
#pragma clang fp contract(off)
                if constexpr (EVAL) {
                    const float omega = (lab ? cw1 : cw0) * pwv[u];
                    float fce, fg;
                    if constexpr (FOCAL) head_focal(lab != 0, l0, l1, m, s, p0, p1, gamma, fce, fg);
                    else fce = head_ce(lab != 0, l0, l1, m, s);
                    lsum = fmaf(fce, omega, lsum);
                    osum += omega;
                }
                sp = fmaf(pwv[u], p1, sp);
                if (lab) {
                    si = fmaf(pwv[u], p1, si);
                    sy += pwv[u];
                }
            }
            if constexpr (EVAL) {
                // p1 is in [0, 1] (or NaN from non-finite logits, which converts to 0): the clamp keeps the index inside the array regardless
                const int bin = max(0, min(EW_EVAL_BINS - 1, (int)(p1 * (float)EW_EVAL_BINS)));
                atomicAdd(&hist[(int)lab * EW_EVAL_BINS + bin], 1u);
            }
        }
    }
    // block reduce: the threads with sub == 0 hold the sums
    __shared__ float red[256 * NS];
    float* my = red + threadIdx.x * NS;
    if constexpr (EVAL) {
        my[0] = lsum;
        my[1] = osum;
    }
    my[NS - 3] = si;
    my[NS - 2] = sp;
    my[NS - 1] = sy;
    __syncthreads();
    if (threadIdx.x < NS) partial[(long)blockIdx.x * NS + threadIdx.x] = head_block_sum<NS>(red, 0, threadIdx.x, ppb, LP);
    if constexpr (EVAL)
        for (int i = threadIdx.x; i < 2 * EW_EVAL_BINS; i += 256) hpart[(long)blockIdx.x * (2 * EW_EVAL_BINS) + i] = hist[i];
}
// one wave per sum, k_head_final's lanes and order; dice_sums[0..2] = {I, P, Y} is OVERWRITTEN (the caller zeroes nothing)
__global__ void __launch_bounds__(256) k_head_final_dice_sums(const float* __restrict__ partial, float* __restrict__ dice_sums, int nblk) {
    const int o = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (o >= 3) return;
    const float t = head_final_sum(partial, nblk, 3, o, lane);
    if (lane == 0) dice_sums[o] = t;
}
// Workgroups 0 and 1: one wave per sum, k_head_final's lanes and order; sums[0..4] ACCUMULATE (+=: a validation set sums on the device).
// Workgroups 2 .. 2 + 8 * EW_EVAL_SLICES - 1: the histogram rows. Workgroup (g, s) owns the 64 bins of group g and the rows
// bk = 4 s + wave (mod 4 * EW_EVAL_SLICES): a wave reads 256 contiguous bytes per row, the four waves meet in LDS, and 64 lanes add the
// slice's 64 totals to hist with one vector 64-bit atomic each (512 contiguous bytes; EW_EVAL_SLICES adds per address per call, whatever
// the input). Integer adds: the result does not depend on their order.
__global__ void __launch_bounds__(256) k_head_eval_final(const float* __restrict__ partial, const unsigned* __restrict__ hpart,
                                                         float* __restrict__ sums, unsigned long long* __restrict__ hist, int nblk) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (blockIdx.x < 2) {
        const int o = blockIdx.x * 4 + wave;
        if (o >= 5) return;
        const float t = head_final_sum(partial, nblk, 5, o, lane);
        if (lane == 0) sums[o] += t;
        return;
    }
    const int hb = blockIdx.x - 2, g = hb & 7, s = hb >> 3;
    unsigned long long t = 0ull;
    for (int bk = 4 * s + wave; bk < nblk; bk += 4 * EW_EVAL_SLICES) t += hpart[(long)bk * (2 * EW_EVAL_BINS) + g * 64 + lane];
    __shared__ unsigned long long acc[4 * 64];
    acc[threadIdx.x] = t;
    __syncthreads();
    if (wave == 0) {
        t = acc[lane] + acc[64 + lane] + acc[128 + lane] + acc[192 + lane];
        if (t) atomicAdd(&hist[g * 64 + lane], t);
    }
}

// ---------------------------------------------------------------------------------------------
// host-side launchers
// ---------------------------------------------------------------------------------------------
int ew_head_blocks(long npix, int C) {
    const int ppb = 256 / (C / 8);
    long nb = (npix + (long)ppb * 8 - 1) / ((long)ppb * 8);
    if (nb > 1024) nb = 1024;
    if (nb < 1) nb = 1;
    return (int)nb;
}
hipError_t ew_head(bool train, const void* act, const float* w, const float* b, const int64_t* labels, float* prob, float* logits, void* dact,
                   float* dw, float* db, float* loss_sum, float* ws, long npix, int C, float inv_count, hipStream_t st) {
    const int nb = ew_head_blocks(npix, C);
    if (train) {
        hipLaunchKernelGGL(k_head<true>, dim3(nb), dim3(256), 0, st, (const bf16_t*)act, w, b, labels, prob, logits, (bf16_t*)dact, ws, npix, C, inv_count);
        hipLaunchKernelGGL(k_head_final, dim3((2 * C + 3 + 3) / 4), dim3(256), 0, st, ws, dw, db, loss_sum, nb, C);
    } else {
        hipLaunchKernelGGL(k_head<false>, dim3(nb), dim3(256), 0, st, (const bf16_t*)act, w, b, nullptr, prob, logits, nullptr, nullptr, npix, C, 0.f);
    }
    return hipGetLastError();
}
template <bool FOCAL, bool DICE>
static auto head_train_kernel(bool aux) { return aux ? k_head_train<FOCAL, DICE, true> : k_head_train<FOCAL, DICE, false>; }
hipError_t hd_train(const void* act, const float* w, const float* b, const int64_t* labels, const float* class_w, const float* pixel_w, float gamma,
                    const float* dice_sums, float dice_scale, float smooth, const float* gprob, float* prob, void* dact, float* dw, float* db,
                    float* loss_sum, float* weight_sum, float* ws, long npix, int C, float inv_count, hipStream_t st) {
    const int nb = ew_head_blocks(npix, C);
    const bool aux = gprob != nullptr;
    auto kern = gamma > 0.f ? (dice_sums ? head_train_kernel<true, true>(aux) : head_train_kernel<true, false>(aux))
                            : (dice_sums ? head_train_kernel<false, true>(aux) : head_train_kernel<false, false>(aux));
    hipLaunchKernelGGL(kern, dim3(nb), dim3(256), 0, st, (const bf16_t*)act, w, b, labels, class_w, pixel_w, gamma, dice_sums, dice_scale, smooth,
                       gprob, prob, (bf16_t*)dact, ws, npix, C, inv_count);
    hipLaunchKernelGGL(k_head_final_loss, dim3((2 * C + 4 + 3) / 4), dim3(256), 0, st, ws, dw, db, loss_sum, weight_sum, nb, C);
    return hipGetLastError();
}
hipError_t ew_head_dice_sums(const void* act, const float* w, const float* b, const int64_t* labels, const float* pixel_w, float* prob,
                             float* dice_sums, float* ws, long npix, int C, hipStream_t st) {
    const int nb = ew_head_blocks(npix, C);
    hipLaunchKernelGGL((k_head_sums<false, false>), dim3(nb), dim3(256), 0, st, (const bf16_t*)act, w, b, labels, nullptr, pixel_w, 0.f, prob, ws,
                       nullptr, npix, C);
    hipLaunchKernelGGL(k_head_final_dice_sums, dim3(1), dim3(256), 0, st, ws, dice_sums, nb);
    return hipGetLastError();
}
size_t ew_head_eval_ws_floats(long npix, int C) { return (size_t)ew_head_blocks(npix, C) * (5 + 2 * EW_EVAL_BINS); }
hipError_t hd_eval(const void* act, const float* w, const float* b, const int64_t* labels, const float* class_w, const float* pixel_w, float gamma,
                   float* prob, float* sums, unsigned long long* hist, float* ws, long npix, int C, hipStream_t st) {
    static_assert(2 * EW_EVAL_BINS == 8 * 64, "k_head_eval_final cuts the histogram into 8 groups of 64 bins");
    const int nb = ew_head_blocks(npix, C);
    unsigned* hpart = (unsigned*)(ws + (size_t)nb * 5);   // [nb][2][EW_EVAL_BINS] behind the [nb][5] partial sums
    hipLaunchKernelGGL((gamma > 0.f ? k_head_sums<true, true> : k_head_sums<true, false>), dim3(nb), dim3(256), 0, st, (const bf16_t*)act, w, b, labels,
                       class_w, pixel_w, gamma, prob, ws, hpart, npix, C);
    hipLaunchKernelGGL(k_head_eval_final, dim3(2 + 8 * EW_EVAL_SLICES), dim3(256), 0, st, ws, hpart, sums, hist, nb);
    return hipGetLastError();
}
