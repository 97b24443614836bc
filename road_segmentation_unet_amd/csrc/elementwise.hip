// HBM-bound kernels of the U-Net path: 16-byte (8 x bf16) accesses per lane everywhere, coalesced along
// the channel axis of NHWC. (The head of the net is head.hip.)
#include "elementwise.h"

// ---------------------------------------------------------------------------------------------
// unet.py:22-23  color_space_adjust
// ---------------------------------------------------------------------------------------------
// tf.nn.dropout (unet.py:29-30, 64-65): y = x / keep * floor(keep + U[0,1)). TensorFlow's Philox stream cannot be reproduced, so
// U comes from a counter-based hash of (key, element index) that the test-side CPU restatement reproduces bit for bit. key = f(seed, dropout site, step) is chosen by the host; element index = NHWC linear index of the tensor being dropped.
__device__ __forceinline__ float drop_keep(unsigned key, unsigned idx, float keep) {
    unsigned h = idx ^ key;
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    const float u = (float)(h >> 8) * (1.0f / 16777216.0f);
    return floorf(keep + u);  // 1 = kept, 0 = dropped
}

// out16 = { dropout(net0)[0..2], 0, m[cj] * (x-0.5)[ci] at 4 + 3*ci + cj, m[0..2] at 13..15 } with m = 1 without dropout
__global__ void k_color_adjust(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                               bf16_t* __restrict__ out16, long npix, float keep, unsigned key) {
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= npix) return;
    const float xc[3] = {x[3 * p] - 0.5f, x[3 * p + 1] - 0.5f, x[3 * p + 2] - 0.5f};
    float m[3] = {1.f, 1.f, 1.f};
    float inv = 1.f;
    if (keep < 1.f) {
        inv = 1.f / keep;
#pragma unroll
        for (int c = 0; c < 3; ++c) m[c] = drop_keep(key, (unsigned)(3 * p + c), keep);
    }
    float f[16];
#pragma unroll
    for (int c = 0; c < 3; ++c) f[c] = fmaf(xc[2], w[6 + c], fmaf(xc[1], w[3 + c], fmaf(xc[0], w[c], b[c]))) * (m[c] * inv);
    f[3] = 0.f;
#pragma unroll
    for (int ci = 0; ci < 3; ++ci)
#pragma unroll
        for (int cj = 0; cj < 3; ++cj) f[4 + 3 * ci + cj] = xc[ci] * m[cj];
#pragma unroll
    for (int cj = 0; cj < 3; ++cj) f[13 + cj] = m[cj];
    u32x4* o = (u32x4*)(out16 + 16 * p);
    o[0] = pack8(f);
    o[1] = pack8(f + 8);
}

// generic dropout of a bf16 tensor (decoder: input of each transposed conv), 8 elements per thread
__global__ void k_dropout(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, long n8, float keep, unsigned key) {
    const float inv = 1.f / keep;
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n8; t += (long)gridDim.x * blockDim.x) {
        float v[8];
        unpack8(*(const u32x4*)(x + 8 * t), v);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] *= drop_keep(key, (unsigned)(8 * t + i), keep) * inv;
        *(u32x4*)(y + 8 * t) = pack8(v);
    }
}

// ---------------------------------------------------------------------------------------------
// level-0 conv1 gradients: rows of the 16-channel wgrad result -> dW1 / colour-adjust helper sums
// ---------------------------------------------------------------------------------------------
__global__ void k_scatter_first_grads(const float* __restrict__ tmp, float* __restrict__ dw1, float* __restrict__ gx, int Cout) {
    // tmp [9][16][Cout] -> dw1 [9][3][Cout] (rows 0..2) and gx [9][12][Cout] (rows 4..15: 9 masked (x-0.5) products, 3 mask sums)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= 9 * 12 * Cout) return;
    const int co = i % Cout, r = i / Cout, row = r % 12, tap = r / 12;
    if (gx) gx[i] = tmp[((long)tap * 16 + 4 + row) * Cout + co];
    if (row < 3) dw1[((long)tap * 3 + row) * Cout + co] = tmp[((long)tap * 16 + row) * Cout + co];
}

// ---------------------------------------------------------------------------------------------
// 2x2 max pool forward
// ---------------------------------------------------------------------------------------------
// `code` (optional, [N][H/2][W/2][C] bytes): per pooled element, bits 0-3 = (window element k > 0) for k = 2*dy + dx, bits 4-5 =
// the window's first maximum in row-major order -- everything the MaxPoolGrad + ReluGrad junction needs from the activation
// (k_pool_skip_relu_bwd then reads one byte per pooled element instead of four bf16 activations)
__global__ void k_maxpool_fwd(const bf16_t* __restrict__ x, bf16_t* __restrict__ y, unsigned char* __restrict__ code, int N, int H, int W, int C,
                              float keep, unsigned key) {
    const float inv = keep < 1.f ? 1.f / keep : 1.f;
    const int Ho = H >> 1, Wo = W >> 1, ncg = C >> 3;
    const long total = (long)N * Ho * Wo * ncg;
    for (long tid = (long)blockIdx.x * blockDim.x + threadIdx.x; tid < total; tid += (long)gridDim.x * blockDim.x) {
        const int cg = (int)(tid % ncg);
        long r = tid / ncg;
        const int ox = (int)(r % Wo);
        r /= Wo;
        const int oy = (int)(r % Ho), n = (int)(r / Ho);
        const bf16_t* p = x + ((long)(n * H + 2 * oy) * W + 2 * ox) * C + cg * 8;
        float a[8], b[8], c[8], d[8];
        unpack8(*(const u32x4*)p, a);
        unpack8(*(const u32x4*)(p + C), b);
        unpack8(*(const u32x4*)(p + (long)W * C), c);
        unpack8(*(const u32x4*)(p + (long)W * C + C), d);
        const long oidx = ((long)(n * Ho + oy) * Wo + ox) * C + cg * 8;
        if (code) {
            unsigned cw[2] = {0u, 0u};
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                int best = 0;
                float m = a[i];
                if (b[i] > m) { m = b[i]; best = 1; }
                if (c[i] > m) { m = c[i]; best = 2; }
                if (d[i] > m) { m = d[i]; best = 3; }
                const unsigned byte = (a[i] > 0.f ? 1u : 0u) | (b[i] > 0.f ? 2u : 0u) | (c[i] > 0.f ? 4u : 0u) | (d[i] > 0.f ? 8u : 0u) | ((unsigned)best << 4);
                cw[i >> 2] |= byte << (8 * (i & 3));
            }
            *(uint2*)(code + oidx) = make_uint2(cw[0], cw[1]);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) a[i] = fmaxf(fmaxf(a[i], b[i]), fmaxf(c[i], d[i]));
        if (keep < 1.f) {  // dropout of the next level's input (unet.py:29-30), fused
#pragma unroll
            for (int i = 0; i < 8; ++i) a[i] *= drop_keep(key, (unsigned)(oidx + i), keep) * inv;
        }
        *(u32x4*)(y + oidx) = pack8(a);
    }
}

// ---------------------------------------------------------------------------------------------
// gradient junction at an encoder output, the training path (code bytes, whole windows, a pooled gradient): one thread = 8 channels
// of one 2x2 window, blockIdx.y = (image, window row), so the index arithmetic is one multiply-high per thread (the general kernel
// below spends ~500 vector instructions per thread on 64-bit divisions and builds float stand-ins of the activation from the code:
// it runs at the vector ALU's pace, 4.6 TB/s alone on the chip and half of that beside a weight-gradient kernel). Same arithmetic:
// dz[k] = (bit k of the code) ? dskip[k] + (k == first maximum ? dpool : 0) : 0, the sum in fp32, rounded once.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_pool_skip_relu_bwd_code(const unsigned char* __restrict__ code, const bf16_t* __restrict__ dpool,
                                                                 const bf16_t* __restrict__ dskip, bf16_t* __restrict__ dz, int N, int H, int W,
                                                                 int C, int Hs, int Ws, unsigned ncg, unsigned ncg_magic, float keep, unsigned key) {
    const int Hp = H >> 1, Wp = W >> 1;
    const unsigned x = blockIdx.x * 256u + threadIdx.x;
    if (x >= (unsigned)Wp * ncg) return;
    unsigned wx = __umulhi(x, ncg_magic), cg = x - wx * ncg;   // floor(2^32 / ncg) may fall one short
    if (cg >= ncg) { ++wx; cg -= ncg; }
    const int oy0 = (H - Hs) / 2, ox0 = (W - Ws) / 2;
  for (int row = (int)blockIdx.y; row < N * Hp; row += (int)gridDim.y) {
    const int n = row / Hp, wy = row - n * Hp;
    const unsigned pidx = (unsigned)(((n * Hp + wy) * Wp + (int)wx) * C) + cg * 8;
    const uint2 c2 = *(const uint2*)(code + pidx);
    const u32x4 dp4 = *(const u32x4*)(dpool + pidx);
    u32x4 g4[4];
    bool have[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int sy = 2 * wy + (k >> 1) - oy0, sx = 2 * (int)wx + (k & 1) - ox0;
        have[k] = dskip && (unsigned)sy < (unsigned)Hs && (unsigned)sx < (unsigned)Ws;
        g4[k] = have[k] ? *(const u32x4*)(dskip + ((long)(n * Hs + sy) * Ws + sx) * C + cg * 8) : u32x4{0u, 0u, 0u, 0u};
    }
    float dp[8];
    unpack8(dp4, dp);
    if (keep < 1.f) {  // the pooled tensor went through dropout: same mask, same scale
        const float inv = 1.f / keep;
#pragma unroll
        for (int i = 0; i < 8; ++i) dp[i] *= drop_keep(key, pidx + i, keep) * inv;
    }
    unsigned best[8], bits[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const unsigned byte = ((i < 4 ? c2.x : c2.y) >> (8 * (i & 3))) & 0xffu;
        best[i] = byte >> 4;
        bits[i] = byte;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float g[8];
        unpack8(g4[k], g);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float v = g[i] + (best[i] == (unsigned)k ? dp[i] : 0.f);
            g[i] = (bits[i] >> k) & 1u ? v : 0.f;
        }
        *(u32x4*)(dz + ((long)(n * H + 2 * wy + (k >> 1)) * W + 2 * (int)wx + (k & 1)) * C + cg * 8) = pack8(g);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// gradient junction at an encoder output: MaxPoolGrad + zero-padded skip gradient + ReluGrad.
// One thread = 8 channels of one 2x2 window.
// ---------------------------------------------------------------------------------------------
__global__ void k_pool_skip_relu_bwd(const bf16_t* __restrict__ yact, const unsigned char* __restrict__ code, const bf16_t* __restrict__ dpool,
                                     const bf16_t* __restrict__ dskip, bf16_t* __restrict__ dz, int N, int H, int W, int C,
                                     int Hs, int Ws, float keep, unsigned key) {
    const float inv = keep < 1.f ? 1.f / keep : 1.f;
    const int Hw = (H + 1) >> 1, Ww = (W + 1) >> 1, ncg = C >> 3;
    const int Hp = H >> 1, Wp = W >> 1;
    const int oy0 = (H - Hs) / 2, ox0 = (W - Ws) / 2;
    const long total = (long)N * Hw * Ww * ncg;
    for (long tid = (long)blockIdx.x * blockDim.x + threadIdx.x; tid < total; tid += (long)gridDim.x * blockDim.x) {
        const int cg = (int)(tid % ncg);
        long r = tid / ncg;
        const int wx = (int)(r % Ww);
        r /= Ww;
        const int wy = (int)(r % Hw), n = (int)(r / Hw);
        float v[4][8], g[4][8];
        bool inb[4];
        // with a code tensor (H, W even: every window is whole) the activation is not read: v[k] = 1 where it was > 0, and 2 at the
        // window's first maximum -- the same comparisons below then pick the same elements
        unsigned cw[2] = {0u, 0u};
        if (code) {
            const uint2 c2 = *(const uint2*)(code + ((long)(n * Hp + wy) * Wp + wx) * C + cg * 8);
            cw[0] = c2.x;
            cw[1] = c2.y;
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int yy = 2 * wy + (k >> 1), xx = 2 * wx + (k & 1);
            inb[k] = (yy < H) && (xx < W);
            if (code) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const unsigned byte = (cw[i >> 2] >> (8 * (i & 3))) & 0xffu;
                    v[k][i] = ((byte >> k) & 1u) ? ((int)(byte >> 4) == k ? 2.f : 1.f) : ((int)(byte >> 4) == k ? 0.f : -1.f);
                }
            } else if (inb[k]) {
                unpack8(*(const u32x4*)(yact + ((long)(n * H + yy) * W + xx) * C + cg * 8), v[k]);
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) v[k][i] = 0.f;
            }
            const int sy = yy - oy0, sx = xx - ox0;
            if (dskip && inb[k] && sy >= 0 && sy < Hs && sx >= 0 && sx < Ws) {
                unpack8(*(const u32x4*)(dskip + ((long)(n * Hs + sy) * Ws + sx) * C + cg * 8), g[k]);
            } else {
#pragma unroll
                for (int i = 0; i < 8; ++i) g[k][i] = 0.f;
            }
        }
        if (dpool && wy < Hp && wx < Wp) {
            float dp[8];
            const long pidx = ((long)(n * Hp + wy) * Wp + wx) * C + cg * 8;
            unpack8(*(const u32x4*)(dpool + pidx), dp);
            if (keep < 1.f) {  // the pooled tensor went through dropout: same mask, same scale
#pragma unroll
                for (int i = 0; i < 8; ++i) dp[i] *= drop_keep(key, (unsigned)(pidx + i), keep) * inv;
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                int best = 0;
                float m = v[0][i];
                if (v[1][i] > m) { m = v[1][i]; best = 1; }
                if (v[2][i] > m) { m = v[2][i]; best = 2; }
                if (v[3][i] > m) { m = v[3][i]; best = 3; }
#pragma unroll
                for (int k = 0; k < 4; ++k) g[k][i] += (best == k) ? dp[i] : 0.f;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!inb[k]) continue;
            const int yy = 2 * wy + (k >> 1), xx = 2 * wx + (k & 1);
#pragma unroll
            for (int i = 0; i < 8; ++i) g[k][i] = v[k][i] > 0.f ? g[k][i] : 0.f;
            *(u32x4*)(dz + ((long)(n * H + yy) * W + xx) * C + cg * 8) = pack8(g[k]);
        }
    }
}

// ---------------------------------------------------------------------------------------------
// BiasAddGrad: per-channel sums over pixels, two deterministic stages
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_colsum_partial(const bf16_t* __restrict__ dz, float* __restrict__ partial, long npix, int C) {
    __shared__ float red[256 * 8];
    const int ncg = C >> 3;
    const int lanes_p = 256 / ncg;  // pixel lanes per block (ncg divides 256)
    const int cg = threadIdx.x % ncg, pl = threadIdx.x / ncg;
    float s[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (pl < lanes_p) {
        for (long p = (long)blockIdx.x * lanes_p + pl; p < npix; p += (long)gridDim.x * lanes_p) {
            float f[8];
            unpack8(*(const u32x4*)(dz + p * C + cg * 8), f);
#pragma unroll
            for (int i = 0; i < 8; ++i) s[i] += f[i];
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) red[threadIdx.x * 8 + i] = s[i];
    __syncthreads();
    for (int c = threadIdx.x; c < C; c += 256) {
        const int g = c >> 3, i = c & 7;
        float t = 0.f;
        for (int q = 0; q < lanes_p; ++q) t += red[(q * ncg + g) * 8 + i];
        partial[(long)blockIdx.x * C + c] = t;
    }
}
// second stage: 32 channels x 8 partial-lanes per block, LDS tree over the lanes (fixed order: deterministic)
__global__ void __launch_bounds__(256) k_colsum_final(const float* __restrict__ partial, float* __restrict__ out, int nblk, int C) {
    __shared__ float red[256];
    const int cl = threadIdx.x & 31, part = threadIdx.x >> 5;
    const int c = blockIdx.x * 32 + cl;
    float t = 0.f;
    if (c < C)
        for (int b = part; b < nblk; b += 8) t += partial[(long)b * C + c];
    red[threadIdx.x] = t;
    __syncthreads();
    if (part == 0 && c < C) {
        float r = 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) r += red[q * 32 + cl];
        out[c] = r;
    }
}

// ---------------------------------------------------------------------------------------------
// split-K slab reduction: out[row][col] = sum_z slab[z][row][col] for the rows of one source
// rows are (tap, cs) pairs: row index -> tap*CsOut + cs_off + cs
// ---------------------------------------------------------------------------------------------
// an optional extra row behind the taps of every slab (column sums of F = bias gradient) is reduced into out2 by the same launch
struct ReduceItem { long e; float* dst; };
__device__ __forceinline__ bool reduce_item(ReduceItem& it, long tid, long total, float* out, float* out2, int n2, int ntap, int CsOut,
                                            int cs_off, int cs_cnt, int CfOut) {
    const int cf4 = CfOut >> 2;
    if (tid < total) {
        const int c4 = (int)(tid % cf4);
        long r = tid / cf4;
        const int cs = (int)(r % cs_cnt), tap = (int)(r / cs_cnt);
        it.e = ((long)tap * CsOut + cs_off + cs) * CfOut + c4 * 4;
        it.dst = out + it.e;
        return true;
    }
    if (out2 && tid < total + n2) {
        const int c4 = (int)(tid - total);
        it.e = (long)ntap * CsOut * CfOut + c4 * 4;
        it.dst = out2 + c4 * 4;
        return true;
    }
    return false;
}
__global__ void k_reduce_slabs(const float* __restrict__ slab, float* __restrict__ out, float* __restrict__ out2, int n2, int nsplit,
                               long slab_elems, int ntap, int CsOut, int cs_off, int cs_cnt, int CfOut) {
    const long total = (long)ntap * cs_cnt * (CfOut >> 2);
    const long total2 = total + (out2 ? n2 : 0);
    for (long tid = (long)blockIdx.x * blockDim.x + threadIdx.x; tid < total2; tid += (long)gridDim.x * blockDim.x) {
        ReduceItem it;
        if (!reduce_item(it, tid, total, out, out2, n2, ntap, CsOut, cs_off, cs_cnt, CfOut)) continue;
        f32x4 t = {0.f, 0.f, 0.f, 0.f};
        for (int z = 0; z < nsplit; ++z) t += *(const f32x4*)(slab + z * slab_elems + it.e);
        *(f32x4*)it.dst = t;
    }
}
// many splits, few outputs: 32 float4 outputs x 8 split-lanes per block, fixed-order LDS tree
__global__ void __launch_bounds__(256) k_reduce_slabs_wide(const float* __restrict__ slab, float* __restrict__ out, float* __restrict__ out2,
                                                           int n2, int nsplit, long slab_elems, int ntap, int CsOut, int cs_off, int cs_cnt,
                                                           int CfOut) {
    __shared__ f32x4 red[256];
    const long total = (long)ntap * cs_cnt * (CfOut >> 2);
    const int el = threadIdx.x & 31, zp = threadIdx.x >> 5;
    const long tid = (long)blockIdx.x * 32 + el;
    f32x4 t = {0.f, 0.f, 0.f, 0.f};
    ReduceItem it;
    const bool have = reduce_item(it, tid, total, out, out2, n2, ntap, CsOut, cs_off, cs_cnt, CfOut);
    if (have)
        for (int z = zp; z < nsplit; z += 8) t += *(const f32x4*)(slab + z * slab_elems + it.e);
    red[threadIdx.x] = t;
    __syncthreads();
    if (zp == 0 && have) {
        f32x4 r = red[el];
#pragma unroll
        for (int q = 1; q < 8; ++q) r += red[q * 32 + el];
        *(f32x4*)it.dst = r;
    }
}

// the slab reductions of a whole group of weight-gradient launches (igemm_wg_group) in ONE launch: block b serves job r with
// block_begin[r] <= b < block_begin[r+1]; per job either form above (wide: 32 outputs x 8 split lanes per block), same summation
// orders as the single launches
__global__ void __launch_bounds__(256) k_reduce_slabs_many(const ReduceJob* __restrict__ jobs, int njobs) {
    __shared__ f32x4 red[256];
    // (njobs <= 16 <= 64 lanes: every lane tests one job, a ballot counts those that begin at or before this block -- one L2 round trip
    // instead of up to 16 dependent ones)
    const int lj = threadIdx.x & 63;
    const bool mine = lj < njobs && jobs[lj].block_begin <= (int)blockIdx.x;
    const int r = __popcll(__ballot(mine)) - 1;
    const ReduceJob J = jobs[r];
    const int b = blockIdx.x - J.block_begin;
    const long total = (long)J.ntap * J.cs_cnt * (J.CfOut >> 2);
    ReduceItem it;
    if (J.wide) {
        const int el = threadIdx.x & 31, zp = threadIdx.x >> 5;
        const long tid = (long)b * 32 + el;
        f32x4 t = {0.f, 0.f, 0.f, 0.f};
        const bool have = reduce_item(it, tid, total, J.out, J.out2, J.n2, J.ntap, J.CsOut, J.cs_off, J.cs_cnt, J.CfOut);
        if (have)
            for (int z = zp; z < J.nsplit; z += 8) t += *(const f32x4*)(J.slab + z * J.slab_elems + it.e);
        red[threadIdx.x] = t;
        __syncthreads();
        if (zp == 0 && have) {
            f32x4 q = red[el];
#pragma unroll
            for (int k = 1; k < 8; ++k) q += red[k * 32 + el];
            *(f32x4*)it.dst = q;
        }
    } else {
        const long tid = (long)b * 256 + threadIdx.x;
        if (!reduce_item(it, tid, total, J.out, J.out2, J.n2, J.ntap, J.CsOut, J.cs_off, J.cs_cnt, J.CfOut)) return;
        f32x4 t = {0.f, 0.f, 0.f, 0.f};
        for (int z = 0; z < J.nsplit; ++z) t += *(const f32x4*)(J.slab + z * J.slab_elems + it.e);
        *(f32x4*)it.dst = t;
    }
}

// color_space_adjust gradients from the first conv's scatter buffer (include/rsu.h, rsu_color_adjust_bwd): 12 outputs, each a
// 9 x Cout sum in a fixed order (lane-strided partials, then an LDS tree): one block of 12 x 64 threads
__global__ void __launch_bounds__(768) k_color_adjust_bwd(const float* __restrict__ gx, const float* __restrict__ w1, float* __restrict__ dW0,
                                                           float* __restrict__ db0, int Cout, float scale, int accumulate) {
    __shared__ float red[12][64];
    const int o = threadIdx.x >> 6, l = threadIdx.x & 63;  // o < 9: dW0[ci][cj] with o = 3*ci + cj; o >= 9: db0[cj]
    const int cj = o < 9 ? o % 3 : o - 9;
    float t = 0.f;
    for (int tap = 0; tap < 9; ++tap)
        for (int co = l; co < Cout; co += 64) t += w1[(tap * 3 + cj) * Cout + co] * gx[(tap * 12 + o) * Cout + co];
    red[o][l] = t;
    __syncthreads();
    if (l == 0) {
        float r = 0.f;
        for (int q = 0; q < 64; ++q) r += red[o][q];
        r *= scale;
        float* dst = o < 9 ? dW0 + o : db0 + (o - 9);
        *dst = accumulate ? *dst + r : r;
    }
}

// ---------------------------------------------------------------------------------------------
// weight packing into MFMA fragment order: packed[chunk][tap][tile][lane][8]
//   element (chunk, tap, tile T, lane, j): row rho = lane&15 of tile T, k = chunk*32 + 8*(lane>>4) + j
//   tile pair P = T/2, t = T%2: output channel of the row = 32P + 8*(rho>>2) + 4t + (rho&3)
//   k runs over the 32-padded concatenation of the K segments (concat sources)
// value = src[tapmap(tap)*s_tap + row*s_row + kreal*s_k]
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void pack_range(const float* __restrict__ src, bf16_t* __restrict__ dst, const PackParams& pp, long e0, long estride) {
    const long total = (long)pp.nchunks * pp.ntap * pp.ntiles * 512;
    for (long e = e0; e < total; e += estride) {
        const int j = (int)(e & 7), lane = (int)((e >> 3) & 63);
        long r = e >> 9;
        const int T = (int)(r % pp.ntiles);
        r /= pp.ntiles;
        const int tap = (int)(r % pp.ntap), chunk = (int)(r / pp.ntap);
        const int rho = lane & 15;
        const int row = 32 * (T >> 1) + 8 * (rho >> 2) + 4 * (T & 1) + (rho & 3);
        int k = chunk * 32 + 8 * (lane >> 4) + j;
        // locate the K segment
        int kreal = -1, base_pad = 0, base_real = 0;
        for (int s = 0; s < pp.nseg; ++s) {
            const int cpad = (pp.seg_c[s] + 31) & ~31;
            if (k >= base_pad && k < base_pad + cpad) {
                const int c = k - base_pad;
                if (c < pp.seg_c[s]) kreal = base_real + c;
            }
            base_pad += cpad;
            base_real += pp.seg_c[s];
        }
        float v = 0.f;
        if (kreal >= 0 && row < pp.rows) {
            const int tsrc = pp.flip ? (pp.ntap - 1 - tap) : tap;
            v = src[(long)tsrc * pp.s_tap + (long)row * pp.s_row + (long)kreal * pp.s_k];
        }
        dst[e] = f2bf(v);
    }
}
__global__ void k_pack(const float* __restrict__ src, bf16_t* __restrict__ dst, PackParams pp) {
    pack_range(src, dst, pp, (long)blockIdx.x * blockDim.x + threadIdx.x, (long)gridDim.x * blockDim.x);
}
// all weight tensors of the network in ONE launch: each job owns a contiguous range of blocks (PACK_EPB elements per block)
#define PACK_EPB 4096
__global__ void __launch_bounds__(256) k_pack_many(const PackJob* __restrict__ jobs, int njobs) {
    __shared__ int sj;
    if (threadIdx.x == 0) {
        int lo = 0, hi = njobs - 1;
        while (lo < hi) {  // last job whose block_start <= blockIdx.x
            const int mid = (lo + hi + 1) >> 1;
            if (jobs[mid].block_start <= (int)blockIdx.x) lo = mid; else hi = mid - 1;
        }
        sj = lo;
    }
    __syncthreads();
    const PackJob jb = jobs[sj];
    const long total = (long)jb.pp.nchunks * jb.pp.ntap * jb.pp.ntiles * 512;
    const long b0 = (long)(blockIdx.x - jb.block_start) * PACK_EPB;
    long hi = b0 + PACK_EPB;
    if (hi > total) hi = total;
    PackParams pp = jb.pp;
    const unsigned g0 = (unsigned)(b0 >> 3), g1 = (unsigned)((hi + 7) >> 3);
    // rows contiguous in the source (HWIO conv kernels packed for the forward pass, the bulk of the bytes): one thread per FOUR
    // neighbouring groups = 4 consecutive rows: eight 16-byte reads (one per k, full sectors) and four 16-byte stores that form
    // one 64-byte run, instead of eight 4-byte reads per group that use a quarter of every sector they touch
    if (pp.s_row == 1 && (pp.rows & 3) == 0 && (pp.s_k & 3) == 0 && (pp.s_tap & 3) == 0 && ((unsigned long)jb.src & 15) == 0 && (g0 & 3) == 0 &&
        (g1 & 3) == 0) {
        for (unsigned q = (g0 >> 2) + threadIdx.x; q < (g1 >> 2); q += 256) {
            const unsigned gidx = q << 2;
            const int lane = (int)(gidx & 63);
            unsigned r = gidx >> 6;
            const int T = (int)(r % (unsigned)pp.ntiles);
            r /= (unsigned)pp.ntiles;
            const int tap = (int)(r % (unsigned)pp.ntap), chunk = (int)(r / (unsigned)pp.ntap);
            const int rho = lane & 15;  // a multiple of 4
            const int row = 32 * (T >> 1) + 8 * (rho >> 2) + 4 * (T & 1);
            const int k0 = chunk * 32 + 8 * (lane >> 4);
            int kreal0 = 0, nvalid = 0, base_pad = 0, base_real = 0;
            for (int sgi = 0; sgi < pp.nseg; ++sgi) {
                const int cpad = (pp.seg_c[sgi] + 31) & ~31;
                if (k0 >= base_pad && k0 < base_pad + cpad) {
                    const int c = k0 - base_pad;
                    kreal0 = base_real + c;
                    nvalid = pp.seg_c[sgi] - c;
                }
                base_pad += cpad;
                base_real += pp.seg_c[sgi];
            }
            if (row >= pp.rows) nvalid = 0;
            const int tsrc = pp.flip ? (pp.ntap - 1 - tap) : tap;
            const float* sp = jb.src + (long)tsrc * pp.s_tap + row + (long)kreal0 * pp.s_k;
            f32x4 v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = j < nvalid ? *(const f32x4*)(sp + (long)j * pp.s_k) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int r3 = 0; r3 < 4; ++r3) {
                const u32x4 o = {pack_bf2(v[0][r3], v[1][r3]), pack_bf2(v[2][r3], v[3][r3]), pack_bf2(v[4][r3], v[5][r3]),
                                 pack_bf2(v[6][r3], v[7][r3])};
                *(u32x4*)(jb.dst + (long)(gidx + r3) * 8) = o;
            }
        }
        return;
    }
    // general case: one thread per 16-byte group (lane, j = 0..7): 32-bit index math once per group, eight strided reads (two 16-byte
    // reads when the k are contiguous in the source), one 16-byte store
    for (unsigned gidx = g0 + threadIdx.x; gidx < g1; gidx += 256) {
        const int lane = (int)(gidx & 63);
        unsigned r = gidx >> 6;
        const int T = (int)(r % (unsigned)pp.ntiles);
        r /= (unsigned)pp.ntiles;
        const int tap = (int)(r % (unsigned)pp.ntap), chunk = (int)(r / (unsigned)pp.ntap);
        const int rho = lane & 15;
        const int row = 32 * (T >> 1) + 8 * (rho >> 2) + 4 * (T & 1) + (rho & 3);
        const int k0 = chunk * 32 + 8 * (lane >> 4);  // the 8 k of a group lie in one (32-padded) segment
        int kreal0 = 0, nvalid = 0, base_pad = 0, base_real = 0;
        for (int sgi = 0; sgi < pp.nseg; ++sgi) {
            const int cpad = (pp.seg_c[sgi] + 31) & ~31;
            if (k0 >= base_pad && k0 < base_pad + cpad) {
                const int c = k0 - base_pad;
                kreal0 = base_real + c;
                nvalid = pp.seg_c[sgi] - c;
            }
            base_pad += cpad;
            base_real += pp.seg_c[sgi];
        }
        if (row >= pp.rows) nvalid = 0;
        const int tsrc = pp.flip ? (pp.ntap - 1 - tap) : tap;
        const float* sp = jb.src + (long)tsrc * pp.s_tap + (long)row * pp.s_row + (long)kreal0 * pp.s_k;
        float v[8];
        if (pp.s_k == 1 && nvalid >= 8 && ((unsigned long)sp & 15) == 0) {
            const f32x4 lo = *(const f32x4*)sp, hi4 = *(const f32x4*)(sp + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                v[j] = lo[j];
                v[4 + j] = hi4[j];
            }
        } else {
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = j < nvalid ? sp[(long)j * pp.s_k] : 0.f;
        }
        const u32x4 o = {pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7])};
        *(u32x4*)(jb.dst + (long)gidx * 8) = o;
    }
}

// ---------------------------------------------------------------------------------------------
// tiler: mirror_border + extract_patches fused (images.py:269-281,35-85), overlap-add (images.py:131-164)
// ---------------------------------------------------------------------------------------------
__global__ void k_extract_tiles(const float* __restrict__ imgs, float* __restrict__ tiles, int H, int S, int P, int stride,
                                int pps, long t0, long ntiles) {
    const int off = (S - P) / 2;
    const long total = ntiles * S * S;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int x = (int)(e % S);
        long r = e / S;
        const int yy = (int)(r % S);
        const long tl = r / S;
        const long tg = t0 + tl;
        const int img = (int)(tg / (pps * pps)), tt = (int)(tg % (pps * pps));
        const int x0 = (tt / pps) * stride, y0 = (tt % pps) * stride;  // x outer, y inner
        int sy = y0 + yy - off, sx = x0 + x - off;                       // coordinates in the un-padded image
        sy = sy < 0 ? -sy - 1 : (sy >= H ? 2 * H - 1 - sy : sy);         // np.pad 'symmetric'
        sx = sx < 0 ? -sx - 1 : (sx >= H ? 2 * H - 1 - sx : sx);
        const float* s = imgs + ((long)(img * H + sy) * H + sx) * 3;
        float* d = tiles + e * 3;
        d[0] = s[0]; d[1] = s[1]; d[2] = s[2];
    }
}

// gather form (deterministic, no atomics): one thread per output pixel sums, in increasing tile index, the tiles of
// [t0, t0+ntiles) that cover it; the in-call sum is kept in double and added to the float accumulator once.
__global__ void k_overlap_add(const float* __restrict__ prob, float* __restrict__ acc, float* __restrict__ hits, int nimg, int H, int P,
                              int stride, int pps, long t0, long ntiles) {
    const long total = (long)nimg * H * H;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int x = (int)(e % H);
        long r = e / H;
        const int y = (int)(r % H), img = (int)(r / H);
        int xi_lo = (x - P + stride) / stride; if (x - P + 1 <= 0) xi_lo = 0;
        int yi_lo = (y - P + stride) / stride; if (y - P + 1 <= 0) yi_lo = 0;
        int xi_hi = x / stride; if (xi_hi > pps - 1) xi_hi = pps - 1;
        int yi_hi = y / stride; if (yi_hi > pps - 1) yi_hi = pps - 1;
        double s = 0.0;
        int cnt = 0;
        for (int xi = xi_lo; xi <= xi_hi; ++xi)
            for (int yi = yi_lo; yi <= yi_hi; ++yi) {
                const long t = (long)img * pps * pps + (long)xi * pps + yi;
                if (t < t0 || t >= t0 + ntiles) continue;
                s += (double)prob[((t - t0) * P + (y - yi * stride)) * P + (x - xi * stride)];
                ++cnt;
            }
        if (cnt) {
            acc[e] += (float)s;
            hits[e] += (float)cnt;
        }
    }
}

__global__ void k_overlap_finish(const float* __restrict__ acc, const float* __restrict__ hits, float* __restrict__ out, long n) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) out[i] = acc[i] / hits[i];
}

// ---- the same tiler for [nimg][H][W] images of any size and any stride (rsu.h "tile grid of an H x W image") ----
// Along an axis of length L: n_reg = (L - P) / stride + 1 regular tiles at i * stride, and, where (L - P) % stride != 0, one clamped tile
// behind them at L - P. The origin of tile i is min(i * stride, L - P) either way.
struct RectAxis {
    int L;       // axis length
    int nreg;    // regular tiles
    int n;       // all tiles: nreg + (clamped ? 1 : 0)
    int last;    // L - P: the clamped tile's origin (the last regular tile's where there is none)
};
static __host__ __device__ inline RectAxis rect_axis(int L, int P, int stride) {
    RectAxis a;
    a.L = L;
    a.last = L - P;
    a.nreg = (L - P) / stride + 1;
    a.n = a.nreg + ((L - P) % stride ? 1 : 0);
    return a;
}
static __device__ inline int rect_origin(const RectAxis& a, int i, int stride) {
    const long o = (long)i * stride;
    return o < a.last ? (int)o : a.last;
}
// np.pad 'symmetric' of any width: period 2L, the second half runs backwards
static __device__ inline int rect_reflect(long c, int L) {
    long m = c % (2L * L);
    if (m < 0) m += 2L * L;
    return (int)(m < L ? m : 2L * L - 1 - m);
}

__global__ void k_extract_tiles_rect(const float* __restrict__ imgs, float* __restrict__ tiles, RectAxis ay, RectAxis ax, int S, int P, int stride,
                                     long t0, long ntiles) {
    const int off = (S - P) / 2;
    const long total = ntiles * S * S, per = (long)ax.n * ay.n;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int x = (int)(e % S);
        long r = e / S;
        const int yy = (int)(r % S);
        const long tg = t0 + r / S;
        const long img = tg / per, tt = tg % per;
        const int x0 = rect_origin(ax, (int)(tt / ay.n), stride), y0 = rect_origin(ay, (int)(tt % ay.n), stride);  // x outer, y inner
        const int sy = rect_reflect((long)y0 + yy - off, ay.L), sx = rect_reflect((long)x0 + x - off, ax.L);
        const float* s = imgs + ((img * ay.L + sy) * ax.L + sx) * 3;
        float* d = tiles + e * 3;
        d[0] = s[0]; d[1] = s[1]; d[2] = s[2];
    }
}

// the regular tiles [lo, hi] of an axis that cover coordinate c (hi < lo: none), and whether the clamped tile does
static __device__ inline void rect_cover(const RectAxis& a, int c, int P, int stride, int& lo, int& hi, int& clamped) {
    lo = c - P + 1 <= 0 ? 0 : (int)(((long)c - P + stride) / stride);
    hi = c / stride;
    if (hi > a.nreg - 1) hi = a.nreg - 1;
    clamped = a.n > a.nreg && c >= a.last;
}

// k_overlap_add's gather with the clamped tiles: per axis the regular tiles in increasing index, then the clamped one (it has the highest
// index), x outer and y inner, so the sum still runs in increasing tile index; double within the call, one float add per call
__global__ void k_overlap_add_rect(const float* __restrict__ prob, float* __restrict__ acc, float* __restrict__ hits, int nimg, RectAxis ay,
                                   RectAxis ax, int P, int stride, long t0, long ntiles) {
    const long total = (long)nimg * ay.L * ax.L, per = (long)ax.n * ay.n;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
        const int x = (int)(e % ax.L);
        long r = e / ax.L;
        const int y = (int)(r % ay.L);
        const long img = r / ay.L;
        int xi_lo, xi_hi, xc, yi_lo, yi_hi, yc;
        rect_cover(ax, x, P, stride, xi_lo, xi_hi, xc);
        rect_cover(ay, y, P, stride, yi_lo, yi_hi, yc);
        double s = 0.0;
        int cnt = 0;
        for (int a = xi_lo; a <= xi_hi + xc; ++a) {
            const int xi = a <= xi_hi ? a : ax.nreg, ox = a <= xi_hi ? a * stride : ax.last;
            for (int b = yi_lo; b <= yi_hi + yc; ++b) {
                const int yi = b <= yi_hi ? b : ay.nreg, oy = b <= yi_hi ? b * stride : ay.last;
                const long t = img * per + (long)xi * ay.n + yi;
                if (t < t0 || t >= t0 + ntiles) continue;
                s += (double)prob[((t - t0) * P + (y - oy)) * P + (x - ox)];
                ++cnt;
            }
        }
        if (cnt) {
            acc[e] += (float)s;
            hits[e] += (float)cnt;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// host-side launchers
// ---------------------------------------------------------------------------------------------
hipError_t ew_color_adjust(const float* x, const float* w, const float* b, void* out16, long npix, float keep, unsigned key, hipStream_t st) {
    hipLaunchKernelGGL(k_color_adjust, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, x, w, b, (bf16_t*)out16, npix, keep, key);
    return hipGetLastError();
}
__global__ void k_scale_bf16(bf16_t* __restrict__ x, long n8, float s) {
    for (long t = (long)blockIdx.x * blockDim.x + threadIdx.x; t < n8; t += (long)gridDim.x * blockDim.x) {
        float v[8];
        unpack8(*(const u32x4*)(x + 8 * t), v);
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] *= s;
        *(u32x4*)(x + 8 * t) = pack8(v);
    }
}
hipError_t ew_scale_bf16(void* x, long n, float s, hipStream_t st) {
    hipLaunchKernelGGL(k_scale_bf16, dim3(grid_for(n / 8, 256)), dim3(256), 0, st, (bf16_t*)x, n / 8, s);
    return hipGetLastError();
}
hipError_t ew_dropout(const void* x, void* y, long n, float keep, unsigned key, hipStream_t st) {
    hipLaunchKernelGGL(k_dropout, dim3(grid_for(n / 8, 256)), dim3(256), 0, st, (const bf16_t*)x, (bf16_t*)y, n / 8, keep, key);
    return hipGetLastError();
}
hipError_t ew_scatter_first_grads(const float* tmp, float* dw1, float* gxc, int Cout, hipStream_t st) {
    hipLaunchKernelGGL(k_scatter_first_grads, dim3((9 * 12 * Cout + 255) / 256), dim3(256), 0, st, tmp, dw1, gxc, Cout);
    return hipGetLastError();
}
hipError_t ew_maxpool_fwd(const void* x, void* y, void* code, int N, int H, int W, int C, float keep, unsigned key, hipStream_t st) {
    const long total = (long)N * (H / 2) * (W / 2) * (C / 8);
    hipLaunchKernelGGL(k_maxpool_fwd, dim3(grid_for(total, 256)), dim3(256), 0, st, (const bf16_t*)x, (bf16_t*)y, (unsigned char*)code, N, H, W, C, keep,
                       key);
    return hipGetLastError();
}
hipError_t ew_pool_skip_relu_bwd(const void* yact, const void* code, const void* dpool, const void* dskip, void* dz, int N, int H, int W, int C,
                                 int Hs, int Ws, float keep, unsigned key, hipStream_t st) {
    if (code && dpool && !((H | W) & 1) && (long)N * H * W * C < (1l << 31)) {   // whole windows, a code byte per pooled element: the lean kernel
        const unsigned ncg = (unsigned)(C / 8), per_row = (unsigned)(W / 2) * ncg;
        const long rows = (long)N * (H / 2);
        hipLaunchKernelGGL(k_pool_skip_relu_bwd_code, dim3((per_row + 255) / 256, (unsigned)(rows < 32768 ? rows : 32768)), dim3(256), 0, st,
                           (const unsigned char*)code, (const bf16_t*)dpool, (const bf16_t*)dskip, (bf16_t*)dz, N, H, W, C, dskip ? Hs : 0, dskip ? Ws : 0, ncg,
                           ncg == 1 ? 0xffffffffu : (unsigned)(0x100000000ull / ncg), keep, key);
        return hipGetLastError();
    }
    const long total = (long)N * ((H + 1) / 2) * ((W + 1) / 2) * (C / 8);
    hipLaunchKernelGGL(k_pool_skip_relu_bwd, dim3(grid_for(total, 256)), dim3(256), 0, st, (const bf16_t*)yact, (const unsigned char*)code,
                       (const bf16_t*)dpool,
                       (const bf16_t*)dskip, (bf16_t*)dz, N, H, W, C, Hs, Ws, keep, key);
    return hipGetLastError();
}
int ew_colsum_blocks(long npix, int C) {
    const int lanes_p = 256 / (C / 8);
    long nb = (npix + (long)lanes_p * 64 - 1) / ((long)lanes_p * 64);
    if (nb > 256) nb = 256;
    if (nb < 1) nb = 1;
    return (int)nb;
}
hipError_t ew_colsum(const void* dz, float* db, float* ws, long npix, int C, hipStream_t st) {
    const int nb = ew_colsum_blocks(npix, C);
    hipLaunchKernelGGL(k_colsum_partial, dim3(nb), dim3(256), 0, st, (const bf16_t*)dz, ws, npix, C);
    hipLaunchKernelGGL(k_colsum_final, dim3((C + 31) / 32), dim3(256), 0, st, ws, db, nb, C);
    return hipGetLastError();
}
hipError_t ew_reduce_slabs(const float* slab, float* out, float* out2, int n2, int nsplit, long slab_elems, int ntap, int CsOut, int cs_off,
                           int cs_cnt, int CfOut, hipStream_t st) {
    const long total = (long)ntap * cs_cnt * (CfOut / 4) + (out2 ? n2 : 0);
    if (nsplit >= 16 && (total + 31) / 32 < 0x7fffffffL)
        hipLaunchKernelGGL(k_reduce_slabs_wide, dim3((unsigned)((total + 31) / 32)), dim3(256), 0, st, slab, out, out2, n2, nsplit, slab_elems, ntap,
                           CsOut, cs_off, cs_cnt, CfOut);
    else
        hipLaunchKernelGGL(k_reduce_slabs, dim3(grid_for(total, 256)), dim3(256), 0, st, slab, out, out2, n2, nsplit, slab_elems, ntap, CsOut,
                           cs_off, cs_cnt, CfOut);
    return hipGetLastError();
}
int ew_reduce_job_blocks(ReduceJob& j) {
    const long total = (long)j.ntap * j.cs_cnt * (j.CfOut / 4) + (j.out2 ? j.n2 : 0);
    j.wide = j.nsplit >= 16 ? 1 : 0;
    return (int)(j.wide ? (total + 31) / 32 : (total + 255) / 256);
}
hipError_t ew_reduce_slabs_many(const ReduceJob* jobs_dev, int njobs, int total_blocks, hipStream_t st) {
    hipLaunchKernelGGL(k_reduce_slabs_many, dim3(total_blocks), dim3(256), 0, st, jobs_dev, njobs);
    return hipGetLastError();
}
hipError_t ew_color_adjust_bwd(const float* gx, const float* w1, float* dW0, float* db0, int Cout, float scale, int accumulate, hipStream_t st) {
    hipLaunchKernelGGL(k_color_adjust_bwd, dim3(1), dim3(768), 0, st, gx, w1, dW0, db0, Cout, scale, accumulate);
    return hipGetLastError();
}
hipError_t ew_pack(const float* src, void* dst, const PackParams& pp, hipStream_t st) {
    const long total = (long)pp.nchunks * pp.ntap * pp.ntiles * 512;
    hipLaunchKernelGGL(k_pack, dim3(grid_for(total, 256)), dim3(256), 0, st, src, (bf16_t*)dst, pp);
    return hipGetLastError();
}
int ew_pack_blocks(const PackParams& pp) {
    const long total = (long)pp.nchunks * pp.ntap * pp.ntiles * 512;
    return (int)((total + PACK_EPB - 1) / PACK_EPB);
}
hipError_t ew_pack_many(const PackJob* jobs_dev, int njobs, int total_blocks, hipStream_t st) {
    hipLaunchKernelGGL(k_pack_many, dim3(total_blocks), dim3(256), 0, st, jobs_dev, njobs);
    return hipGetLastError();
}
hipError_t ew_extract_tiles(const float* imgs, float* tiles, int H, int S, int P, int stride, int pps, long t0, long ntiles, hipStream_t st) {
    hipLaunchKernelGGL(k_extract_tiles, dim3(grid_for(ntiles * S * S, 256)), dim3(256), 0, st, imgs, tiles, H, S, P, stride, pps, t0, ntiles);
    return hipGetLastError();
}
hipError_t ew_overlap_add(const float* prob, float* acc, float* hits, int nimg, int H, int P, int stride, int pps, long t0, long ntiles, hipStream_t st) {
    hipLaunchKernelGGL(k_overlap_add, dim3(grid_for((long)nimg * H * H, 256)), dim3(256), 0, st, prob, acc, hits, nimg, H, P, stride, pps, t0, ntiles);
    return hipGetLastError();
}
hipError_t ew_overlap_finish(const float* acc, const float* hits, float* out, long n, hipStream_t st) {
    hipLaunchKernelGGL(k_overlap_finish, dim3(grid_for(n, 256)), dim3(256), 0, st, acc, hits, out, n);
    return hipGetLastError();
}
void ew_tile_grid(int H, int W, int P, int stride, int* ny, int* nx) {
    *ny = rect_axis(H, P, stride).n;
    *nx = rect_axis(W, P, stride).n;
}
hipError_t ew_extract_tiles_rect(const float* imgs, float* tiles, int H, int W, int S, int P, int stride, long t0, long ntiles, hipStream_t st) {
    hipLaunchKernelGGL(k_extract_tiles_rect, dim3(grid_for(ntiles * S * S, 256)), dim3(256), 0, st, imgs, tiles, rect_axis(H, P, stride),
                       rect_axis(W, P, stride), S, P, stride, t0, ntiles);
    return hipGetLastError();
}
hipError_t ew_overlap_add_rect(const float* prob, float* acc, float* hits, int nimg, int H, int W, int P, int stride, long t0, long ntiles,
                               hipStream_t st) {
    hipLaunchKernelGGL(k_overlap_add_rect, dim3(grid_for((long)nimg * H * W, 256)), dim3(256), 0, st, prob, acc, hits, nimg,
                       rect_axis(H, P, stride), rect_axis(W, P, stride), P, stride, t0, ntiles);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// post-processing (src/images.py:88-99, 256-266; src/summary.py:134-147)
// ---------------------------------------------------------------------------------------------
// One 256-thread workgroup per patch_size x patch_size block of a mask [nimg][S][S] (patch_size <= 64): the block statistic
//   mode 0 (quantize_mask, images.py:256-266):       label = mean(mask >= 0.5) > threshold, written over the whole block of `out`
//   mode 1 (labels_for_patches, images.py:88-99):    label = mean(mask) > threshold, written to labels[img][bx][by] (x outer: the
//                                                    patch order of extract_patches) as int64
// Blocks cut by the image edge average over the pixels they hold (numpy slicing does the same).
// (mask and out may be the SAME buffer -- quantize_mask in place, rsu.h: no __restrict__ on them; a block's stores follow the barrier of
// its reduction, and blocks do not overlap)
__global__ void __launch_bounds__(256) k_block_label(const float* mask, float* out, int64_t* __restrict__ labels,
                                                     int S, int ps, int nb, float thr, int mode) {
    const int b = blockIdx.x, by = b % nb, bx = (b / nb) % nb, img = b / (nb * nb);
    const int y0 = by * ps, x0 = bx * ps;
    const int hh = min(ps, S - y0), ww = min(ps, S - x0);
    float sum = 0.f;
    for (int i = threadIdx.x; i < hh * ww; i += 256) {
        const float v = mask[((long)img * S + y0 + i / ww) * S + x0 + i % ww];
        sum += mode == 0 ? (v >= 0.5f ? 1.f : 0.f) : v;
    }
    __shared__ float red[256];
    red[threadIdx.x] = sum;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const float lab = (red[0] / (float)(hh * ww)) > thr ? 1.f : 0.f;
    if (mode == 0) {
        for (int i = threadIdx.x; i < hh * ww; i += 256) out[((long)img * S + y0 + i / ww) * S + x0 + i % ww] = lab;
    } else if (threadIdx.x == 0) {
        labels[((long)img * nb + bx) * nb + by] = (int64_t)lab;
    }
}
hipError_t ew_block_label(const float* mask, float* out, int64_t* labels, int nimg, int S, int ps, float thr, int mode, hipStream_t st) {
    const int nb = (S + ps - 1) / ps;
    hipLaunchKernelGGL(k_block_label, dim3(nimg * nb * nb), dim3(256), 0, st, mask, out, labels, S, ps, nb, thr, mode);
    return hipGetLastError();
}
// k_block_label's mode 0 on a mask [nimg][H][W]: the same per-thread sums, reduction and rule, with a block grid of nby x nbx
// (mask and out may be the same buffer, as there)
__global__ void __launch_bounds__(256) k_block_label_rect(const float* mask, float* out, int H, int W, int ps, int nby, int nbx, float thr) {
    const int b = blockIdx.x, by = b % nby, bx = (b / nby) % nbx;
    const long img = b / (nby * nbx);
    const int y0 = by * ps, x0 = bx * ps;
    const int hh = min(ps, H - y0), ww = min(ps, W - x0);
    float sum = 0.f;
    for (int i = threadIdx.x; i < hh * ww; i += 256) sum += mask[(img * H + y0 + i / ww) * W + x0 + i % ww] >= 0.5f ? 1.f : 0.f;
    __shared__ float red[256];
    red[threadIdx.x] = sum;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const float lab = (red[0] / (float)(hh * ww)) > thr ? 1.f : 0.f;
    for (int i = threadIdx.x; i < hh * ww; i += 256) out[(img * H + y0 + i / ww) * W + x0 + i % ww] = lab;
}
hipError_t ew_block_label_rect(const float* mask, float* out, int nimg, int H, int W, int ps, float thr, hipStream_t st) {
    const int nby = (H + ps - 1) / ps, nbx = (W + ps - 1) / ps;
    hipLaunchKernelGGL(k_block_label_rect, dim3((unsigned)((long)nimg * nby * nbx)), dim3(256), 0, st, mask, out, H, W, ps, nby, nbx, thr);
    return hipGetLastError();
}
// tf.metrics.{accuracy, recall, precision} counters (summary.py:141-147): counts[0..3] += TP, FP, FN, TN over n int64 labels
__global__ void __launch_bounds__(256) k_confusion(const int64_t* __restrict__ pred, const int64_t* __restrict__ truth, long n,
                                                   unsigned long long* __restrict__ counts) {
    unsigned c[4] = {0, 0, 0, 0};
    for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const int pr = pred[i] != 0, t = truth[i] != 0;
        ++c[pr ? (t ? 0 : 1) : (t ? 2 : 3)];
    }
    __shared__ unsigned red[4][256];
    for (int k = 0; k < 4; ++k) red[k][threadIdx.x] = c[k];
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s)
            for (int k = 0; k < 4; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x < 4) atomicAdd(&counts[threadIdx.x], (unsigned long long)red[threadIdx.x][0]);
}
hipError_t ew_confusion(const int64_t* pred, const int64_t* truth, long n, unsigned long long* counts, hipStream_t st) {
    int grid = (int)((n + 255) / 256);
    if (grid > 1024) grid = 1024;
    hipLaunchKernelGGL(k_confusion, dim3(grid), dim3(256), 0, st, pred, truth, n, counts);
    return hipGetLastError();
}
