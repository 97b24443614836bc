#include "lovasz.h"

// The Lovasz term (include/rsu_lovasz.h; Berman, Triki and Blaschko, CVPR 2018) of a prob map against binary labels, per image:
//   e_i = |y_i - p_i|, ranked by the unsigned bit pattern of e descending, ties by ascending pixel index; c_k = the y = 1 pixels among
//   ranks 1..k; J_k = 1 - (G - c_k) / (G + k - c_k); g_k = J_k - J_{k-1}; L = sum_k e_(k) g_k; d L / d p_i = -+ g_{r(i)}.
// float32 with one rounding per operation: this file is compiled with -ffp-contract=off and hostio.lovasz_gradient restates it bit for bit.
//
// The sort is a bitonic network over 64-bit keys, unique among the counted pixels of an image:
//   bits 63..32 the pattern of e (below 2^31), bit 25 set (a counted pixel's key is never 0), bits 24..1 = 2^24 - 1 - pixel index, bit 0 = y
// so "descending by key" is the order of the header, and the payload (index, label) rides inside the key. Ignored pixels and the padding
// of an image's segment up to Pn = max(LV_TILE, next power of two) hold key 0 and end up behind the n counted pixels. The network for
// position i of an image (standard: for k = 2, 4 .. Pn, for j = k / 2 .. 1: compare i with i ^ j) sorts DESCENDING where (i & k) == 0.
//   k_lv_local<true>   builds the keys of a tile of LV_TILE positions (and writes +0 to gprob at ignored pixels) and runs k = 2 .. LV_TILE
//   k_lv_global<R>     R consecutive steps j >= LV_TILE of one k through global memory: a thread owns the 2^R keys that differ in those
//                      R index bits, so the steps between them need no other thread
//   k_lv_local<false>  the steps j = LV_TILE / 2 .. 1 of one k > LV_TILE
// Inside a tile the steps j >= 8 go through LDS (up to three per barrier, by the same ownership), j = 4, 2, 1 through the 8 registers a
// thread holds. Every k_lv_local also leaves the tile's two counts {y = 1, counted}; those of the last one stand. k_lv_grad then takes a
// tile of ranks: G and the y = 1 pixels in front of the tile from the counts (integers: the order of these sums is immaterial), a scan of y inside the tile, J_k,
// g_k, the products summed in a fixed order, and the scatter of the gradient through the index in the key. k_lv_final adds the tiles'
// sums per image and the images in order. Every trip count is a function of B, H, W; no atomics; nothing waits on another workgroup.
typedef unsigned long long lvkey;
constexpr int LV_THREADS = 512;
constexpr int LV_PER = LV_TILE / LV_THREADS;   // 8 keys per thread
static_assert(LV_PER == 8 && LV_THREADS == 512, "the register steps below are written for 8 keys per thread");

// the two ends of a comparator: the larger key comes first where the run is descending
__device__ __forceinline__ void lv_cmpx(lvkey& a, lvkey& b, bool desc) {
    const lvkey x = a, y = b;
    const bool sw = (x < y) == desc;
    a = sw ? y : x;
    b = sw ? x : y;
}
// the step j = J (4, 2 or 1) of stage k on the 8 consecutive keys at positions i0 .. i0 + 7 of the image
template <int J>
__device__ __forceinline__ void lv_reg_step(lvkey (&v)[LV_PER], unsigned i0, unsigned k) {
#pragma unroll
    for (int m = 0; m < LV_PER; ++m)
        if (!(m & J)) lv_cmpx(v[m], v[m | J], ((i0 + m) & k) == 0);
}
// R steps of stage k, strides sl << (R - 1) .. sl (all >= 8, all < k), on the tile in LDS: a thread takes 8 >> R groups of the 2^R keys
// that differ in those R index bits (k_lv_global's ownership inside a tile), so one barrier serves R steps
template <int R>
__device__ __forceinline__ void lv_lds_phase(lvkey* s, unsigned tile0, unsigned k, unsigned sl) {
#pragma unroll
    for (int u = 0; u < (LV_PER >> R); ++u) {
        const unsigned q = threadIdx.x + LV_THREADS * u, lo = q & (sl - 1), base = ((q - lo) << R) + lo;
        const bool desc = ((tile0 + base) & k) == 0;
        lvkey w[1 << R];
#pragma unroll
        for (int m = 0; m < (1 << R); ++m) w[m] = s[base + m * sl];
#pragma unroll
        for (int sft = R - 1; sft >= 0; --sft)
#pragma unroll
            for (int m = 0; m < (1 << R); ++m)
                if (!(m & (1 << sft))) lv_cmpx(w[m], w[m | (1 << sft)], desc);
#pragma unroll
        for (int m = 0; m < (1 << R); ++m) s[base + m * sl] = w[m];
    }
    __syncthreads();
}
// the steps j = jfirst .. 8 of stage k on the tile in LDS (the caller has stored and synchronised) -- first the one or two strides that
// do not fill a group of three, then three per barrier -- and j = 4, 2, 1 in registers; on return v holds the thread's keys and the LDS
// tile is stale
__device__ __forceinline__ void lv_tile_steps(lvkey* s, lvkey (&v)[LV_PER], unsigned tile0, unsigned k, unsigned jfirst) {
    const unsigned tid = threadIdx.x;
    unsigned j = jfirst;
    const int rest = (__builtin_ctz(j) - 2) % 3;   // (strides j .. 8: ctz(j) - 2 of them)
    if (rest == 1) {
        lv_lds_phase<1>(s, tile0, k, j);
        j >>= 1;
    } else if (rest == 2) {
        lv_lds_phase<2>(s, tile0, k, j >> 1);
        j >>= 2;
    }
    for (; j >= 8; j >>= 3) lv_lds_phase<3>(s, tile0, k, j >> 2);
#pragma unroll
    for (int m = 0; m < LV_PER; ++m) v[m] = s[tid * LV_PER + m];
    const unsigned i0 = tile0 + tid * LV_PER;
    lv_reg_step<4>(v, i0, k);
    lv_reg_step<2>(v, i0, k);
    lv_reg_step<1>(v, i0, k);
}

template <bool BUILD>
__global__ void __launch_bounds__(LV_THREADS) k_lv_local(lvkey* __restrict__ keys, const float* __restrict__ prob,
                                                         const int64_t* __restrict__ labels, float* __restrict__ gprob, int accumulate,
                                                         int* __restrict__ counts, unsigned HW, unsigned tiles_per_image, unsigned k) {
#pragma clang fp contract(off)
    __shared__ lvkey s[LV_TILE];
    __shared__ int red[2 * LV_THREADS];
    const unsigned tid = threadIdx.x;
    const unsigned b = blockIdx.x / tiles_per_image, tile0 = (blockIdx.x % tiles_per_image) * LV_TILE;
    lvkey* seg = keys + (size_t)blockIdx.x * LV_TILE;   // (= image b's segment + tile0)
    lvkey v[LV_PER];
    if (BUILD) {
        const unsigned i0 = tile0 + tid * LV_PER;
#pragma unroll
        for (int m = 0; m < LV_PER; ++m) {
            const unsigned i = i0 + m;
            lvkey key = 0;
            if (i < HW) {
                const size_t g = (size_t)b * HW + i;
                const int64_t lab = labels[g];
                if (lab == 0 || lab == 1) {
                    const float e = fabsf((float)lab - prob[g]);
                    key = ((lvkey)__float_as_uint(e) << 32) | (1u << 25) | ((0xFFFFFFu - i) << 1) | (unsigned)lab;
                } else if (gprob) {
                    gprob[g] = accumulate ? gprob[g] + 0.f : 0.f;   // an ignored pixel: +0, its p is not looked at
                }
            }
            v[m] = key;
        }
        lv_reg_step<1>(v, i0, 2);
        lv_reg_step<2>(v, i0, 4);
        lv_reg_step<1>(v, i0, 4);
        lv_reg_step<4>(v, i0, 8);
        lv_reg_step<2>(v, i0, 8);
        lv_reg_step<1>(v, i0, 8);
        for (unsigned kk = 16; kk <= LV_TILE; kk <<= 1) {
#pragma unroll
            for (int m = 0; m < LV_PER; ++m) s[tid * LV_PER + m] = v[m];
            __syncthreads();
            lv_tile_steps(s, v, tile0, kk, kk >> 1);
            __syncthreads();   // (every thread has read its keys back before the next stage stores)
        }
    } else {
#pragma unroll
        for (int m = 0; m < LV_PER; ++m) s[tid * LV_PER + m] = seg[tid * LV_PER + m];
        __syncthreads();
        lv_tile_steps(s, v, tile0, k, LV_TILE / 2);
    }
    int cy = 0, cn = 0;
#pragma unroll
    for (int m = 0; m < LV_PER; ++m) {
        seg[tid * LV_PER + m] = v[m];
        cy += (int)(v[m] & 1);
        cn += v[m] != 0;
    }
    red[tid] = cy;
    red[LV_THREADS + tid] = cn;
    __syncthreads();
    for (unsigned st = LV_THREADS / 2; st > 0; st >>= 1) {
        if (tid < st) {
            red[tid] += red[tid + st];
            red[LV_THREADS + tid] += red[LV_THREADS + tid + st];
        }
        __syncthreads();
    }
    if (tid == 0) {
        counts[2 * (size_t)blockIdx.x] = red[0];
        counts[2 * (size_t)blockIdx.x + 1] = red[LV_THREADS];
    }
}

// R steps of stage k, strides jl << (R - 1) .. jl (all >= LV_TILE, all < k): thread q of an image owns positions base + m * jl, m < 2^R.
// Pn >> R is a multiple of the workgroup's 256 threads (Pn >= 2 LV_TILE), so the grid is exact and no thread is idle.
template <int R>
__global__ void __launch_bounds__(256) k_lv_global(lvkey* __restrict__ keys, unsigned Pn, unsigned k, unsigned jl) {
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    const unsigned per = Pn >> R;
    const size_t b = q / per;
    const unsigned r = (unsigned)(q % per), lo = r & (jl - 1), base = ((r - lo) << R) + lo;
    lvkey* p = keys + b * Pn + base;
    const bool desc = (base & k) == 0;
    lvkey v[1 << R];
#pragma unroll
    for (int m = 0; m < (1 << R); ++m) v[m] = p[(size_t)m * jl];
#pragma unroll
    for (int sft = R - 1; sft >= 0; --sft)
#pragma unroll
        for (int m = 0; m < (1 << R); ++m)
            if (!(m & (1 << sft))) lv_cmpx(v[m], v[m | (1 << sft)], desc);
#pragma unroll
    for (int m = 0; m < (1 << R); ++m) p[(size_t)m * jl] = v[m];
}

// one tile of LV_TILE ranks of an image: positions pos = tile0 + 8 tid + m hold rank k = pos + 1
__global__ void __launch_bounds__(LV_THREADS) k_lv_grad(const lvkey* __restrict__ keys, const int* __restrict__ counts,
                                                        float* __restrict__ partial, float* __restrict__ gprob, int accumulate, float c,
                                                        unsigned HW, unsigned tiles_per_image) {
#pragma clang fp contract(off)
    __shared__ int sc[2][LV_THREADS];
    __shared__ int red[3 * LV_THREADS];
    __shared__ float fr[LV_THREADS];
    const unsigned tid = threadIdx.x;
    const unsigned b = blockIdx.x / tiles_per_image, t = blockIdx.x % tiles_per_image, tile0 = t * LV_TILE;
    const lvkey* seg = keys + (size_t)blockIdx.x * LV_TILE;
    // G and the y = 1 pixels in front of this tile (integers: any order)
    int G = 0, before = 0;
    for (unsigned u = tid; u < tiles_per_image; u += LV_THREADS) {
        const int cy = counts[2 * ((size_t)b * tiles_per_image + u)];
        G += cy;
        before += u < t ? cy : 0;
    }
    lvkey v[LV_PER];
    int ys = 0;
#pragma unroll
    for (int m = 0; m < LV_PER; ++m) {
        v[m] = seg[tid * LV_PER + m];
        ys += (int)(v[m] & 1);
    }
    red[tid] = G;
    red[LV_THREADS + tid] = before;
    sc[0][tid] = ys;
    __syncthreads();
    for (unsigned st = LV_THREADS / 2; st > 0; st >>= 1) {
        if (tid < st) {
            red[tid] += red[tid + st];
            red[LV_THREADS + tid] += red[LV_THREADS + tid + st];
        }
        __syncthreads();
    }
    G = red[0];
    before = red[LV_THREADS];
    // inclusive scan of the threads' y counts (Hillis-Steele between two buffers)
    int cur = 0;
    for (unsigned d = 1; d < LV_THREADS; d <<= 1) {
        sc[cur ^ 1][tid] = sc[cur][tid] + (tid >= d ? sc[cur][tid - d] : 0);
        cur ^= 1;
        __syncthreads();
    }
    int ck = before + sc[cur][tid] - ys;   // c_{k-1} of the thread's first rank
    float acc = 0.f;
#pragma unroll
    for (int m = 0; m < LV_PER; ++m) {
        const lvkey key = v[m];
        float prod = 0.f;
        if (key != 0) {   // a counted pixel: rank k <= n
            const int k = (int)(tile0 + tid * LV_PER + m) + 1, y = (int)(key & 1);
            const int cprev = ck;
            ck += y;
            const float jk = 1.f - (float)(G - ck) / (float)(G + k - ck);
            const float jprev = k > 1 ? 1.f - (float)(G - cprev) / (float)(G + (k - 1) - cprev) : 0.f;
            const float g = jk - jprev;
            prod = __uint_as_float((unsigned)(key >> 32)) * g;
            if (gprob) {
                const unsigned idx = 0xFFFFFFu - ((unsigned)(key >> 1) & 0xFFFFFFu);
                const float cg = c * g;
                const float val = y ? -cg : cg;
                float* dst = gprob + (size_t)b * HW + idx;   // (idx < HW: only pixels of the image were given a key)
                *dst = accumulate ? *dst + val : val;
            }
        }
        acc = acc + prod;
    }
    fr[tid] = acc;
    __syncthreads();
    for (unsigned st = LV_THREADS / 2; st > 0; st >>= 1) {
        if (tid < st) fr[tid] = fr[tid] + fr[tid + st];
        __syncthreads();
    }
    if (tid == 0) partial[blockIdx.x] = fr[0];
}

// L_b: thread i adds the tiles i, i + 256, .. of image b in order, a binary tree adds the threads; thread 0 adds the images in order
__global__ void __launch_bounds__(256) k_lv_final(const float* __restrict__ partial, float* __restrict__ loss_sum, int B,
                                                  unsigned tiles_per_image) {
#pragma clang fp contract(off)
    __shared__ float fr[256];
    const unsigned tid = threadIdx.x;
    float total = 0.f;
    for (int b = 0; b < B; ++b) {
        float a = 0.f;
        for (unsigned u = tid; u < tiles_per_image; u += 256) a = a + partial[(size_t)b * tiles_per_image + u];
        fr[tid] = a;
        __syncthreads();
        for (unsigned st = 128; st > 0; st >>= 1) {
            if (tid < st) fr[tid] = fr[tid] + fr[tid + st];
            __syncthreads();
        }
        total = total + fr[0];
        __syncthreads();
    }
    if (tid == 0) {
        loss_sum[0] = loss_sum[0] + total;
        loss_sum[1] = loss_sum[1] + (float)B;
    }
}

long lv_padded(int H, int W) {
    const long hw = (long)H * W;
    long p = LV_TILE;
    while (p < hw) p <<= 1;
    return p;
}
static int lv_log2(long p) {
    int l = 0;
    while ((1l << l) < p) ++l;
    return l;
}
size_t lv_ws_bytes(int B, int H, int W) {
    const size_t keys = (size_t)B * (size_t)lv_padded(H, W);
    return keys * 8 + keys / LV_TILE * 12;
}
hipError_t lv_run(const float* prob, const int64_t* labels, float c, int accumulate, float* gprob, float* loss_sum, void* ws, int B, int H,
                  int W, hipStream_t st) {
    const unsigned HW = (unsigned)(H * W), Pn = (unsigned)lv_padded(H, W), tpi = Pn / LV_TILE;
    const size_t nkeys = (size_t)B * Pn, tiles = nkeys / LV_TILE;
    lvkey* keys = (lvkey*)ws;
    int* counts = (int*)(keys + nkeys);
    float* partial = (float*)(counts + 2 * tiles);
    hipLaunchKernelGGL(k_lv_local<true>, dim3((unsigned)tiles), dim3(LV_THREADS), 0, st, keys, prob, labels, gprob, accumulate, counts, HW, tpi,
                       0u);
    for (unsigned k = 2 * LV_TILE; k <= Pn && k != 0; k <<= 1) {
        unsigned j = k >> 1;   // the next stride; the strides LV_TILE .. j are left for global memory
        while (j >= (unsigned)LV_TILE) {
            const unsigned left = (unsigned)lv_log2(j / LV_TILE) + 1, R = left >= 3 ? 3 : left, jl = j >> (R - 1);
            const dim3 grid((unsigned)((nkeys >> R) / 256));
            if (R == 3) hipLaunchKernelGGL(k_lv_global<3>, grid, dim3(256), 0, st, keys, Pn, k, jl);
            else if (R == 2) hipLaunchKernelGGL(k_lv_global<2>, grid, dim3(256), 0, st, keys, Pn, k, jl);
            else hipLaunchKernelGGL(k_lv_global<1>, grid, dim3(256), 0, st, keys, Pn, k, jl);
            j = jl >> 1;
        }
        hipLaunchKernelGGL(k_lv_local<false>, dim3((unsigned)tiles), dim3(LV_THREADS), 0, st, keys, (const float*)nullptr,
                           (const int64_t*)nullptr, (float*)nullptr, 0, counts, HW, tpi, k);
    }
    hipLaunchKernelGGL(k_lv_grad, dim3((unsigned)tiles), dim3(LV_THREADS), 0, st, keys, counts, partial, gprob, accumulate, c, HW, tpi);
    hipLaunchKernelGGL(k_lv_final, dim3(1), dim3(256), 0, st, partial, loss_sum, B, tpi);
    return hipGetLastError();
}
