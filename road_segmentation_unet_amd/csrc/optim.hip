// The optimizer step's kernels: the Momentum and Adam rules, the one-pass update + bf16 re-pack over a job table, the gradient's global
// norm, the moving average of the weights and gradient accumulation. All HBM-bound: 16-byte accesses per lane, full 128-byte rows.
#include "optim.h"

// ---------------------------------------------------------------------------------------------
// Adam (tf.train.AdamOptimizer, TensorFlow 1.x ApplyAdam): the per-element update of rsu_adam_step and of the Adam instantiation of
// k_update_pack_many -- ONE function, so both give the same bits. float32 in TensorFlow's operation order, IEEE sqrt and divide, no
// contraction (an FMA where ApplyAdam rounds twice would move the last bit between this kernel and a float32 restatement).
// alpha = lr_t * sqrt(1 - beta2^t) / (1 - beta1^t) comes from the host (AdamRule).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void adam_elem(float& w, float& m, float& v, float g, const AdamRule& h) {
#pragma clang fp contract(off)
    const float gs = h.gscale * g;
    m += (gs - m) * (1.f - h.beta1);
    v += (gs * gs - v) * (1.f - h.beta2);
    w -= (m * h.alpha) / (sqrtf(v) + h.epsilon);
}
__device__ __forceinline__ void adam_elem4(f32x4& w, f32x4& m, f32x4& v, const f32x4 g, const AdamRule& h) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float wj = w[j], mj = m[j], vj = v[j];
        adam_elem(wj, mj, vj, g[j], h);
        w[j] = wj; m[j] = mj; v[j] = vj;
    }
}
__global__ void k_adam(float* __restrict__ w, float* __restrict__ m, float* __restrict__ v, const float* __restrict__ g, AdamRule h, long n) {
    const long n4 = n >> 2;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        f32x4 mv = ((f32x4*)m)[i], vv = ((f32x4*)v)[i], gv = ((const f32x4*)g)[i], wv = ((f32x4*)w)[i];
        adam_elem4(wv, mv, vv, gv, h);
        ((f32x4*)m)[i] = mv;
        ((f32x4*)v)[i] = vv;
        ((f32x4*)w)[i] = wv;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const long i = (n4 << 2) + threadIdx.x;
        adam_elem(w[i], m[i], v[i], g[i], h);
    }
}

// ---------------------------------------------------------------------------------------------
// momentum SGD (tf_aerial_images.py:116-121)
// ---------------------------------------------------------------------------------------------
__global__ void k_momentum(float* __restrict__ w, float* __restrict__ acc, const float* __restrict__ g, float lr, float mu, float gscale, long n) {
    const long n4 = n >> 2;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        f32x4 a = ((f32x4*)acc)[i], gv = ((const f32x4*)g)[i], wv = ((f32x4*)w)[i];
        a = mu * a + gscale * gv;
        wv -= lr * a;
        ((f32x4*)acc)[i] = a;
        ((f32x4*)w)[i] = wv;
    }
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const long i = (n4 << 2) + threadIdx.x;
        const float a = mu * acc[i] + gscale * g[i];
        acc[i] = a;
        w[i] -= lr * a;
    }
}

// ---------------------------------------------------------------------------------------------
// Momentum step + re-pack in ONE pass over the parameters (k_update_pack_many). k_momentum moves 20 B per parameter and k_pack_many
// reads every conv kernel twice more (once per packed layout, 12 B per weight, at half the copy rate: its gathers use a quarter of
// a sector for one of the two layouts). Here a workgroup owns 32 x 128 source elements of one tap of one tensor -- four 32 x 32
// blocks: it reads w, acc, g once (full 128-byte rows), updates them, keeps the new weights in LDS and writes BOTH packed layouts
// from there, each block as one contiguous 2-KiB run of 16-byte pieces: 24 B per weight, every access a full sector. Small
// variables that no MFMA kernel reads (biases, colour adjust, the 1x1 head) are plain ranges of the same launch.
// Source tensor = [ntap][R1][R2] float32, R2 contiguous (conv kernels HWIO: R1 = ci, R2 = co; transposed-conv kernels
// [a][b][co][ci]: R1 = co, R2 = ci). A packed layout is [chunk of 32 k][tap][16-row tile][lane][8] (pack_range, elementwise.hip); a
// destination takes its ROWS from R2 and k from R1 ("orientation A": conv forward, transposed-conv backward) or rows from R1 and k
// from R2 ("B": conv backward-data, one buffer per concat source; transposed-conv forward, one buffer per tap).
// ---------------------------------------------------------------------------------------------
#define UP_EPB 4096   // floats per workgroup of a plain range
namespace {
// the update rules of the pass, on a float4 of weights (w, first slot a, second slot v, gradient g)
__device__ __forceinline__ void up_step(const MomentumRule& h, f32x4& w, f32x4& a, f32x4&, const f32x4 g) {
    a = h.mu * a + h.gscale * g;
    w -= h.lr * a;
}
__device__ __forceinline__ void up_step(const AdamRule& h, f32x4& w, f32x4& a, f32x4& v, const f32x4 g) { adam_elem4(w, a, v, g, h); }
__device__ __forceinline__ void up_step1(const MomentumRule& h, float* w, float* a, float*, const float* g) {
    const float an = h.mu * *a + h.gscale * *g;
    *a = an;
    *w -= h.lr * an;
}
__device__ __forceinline__ void up_step1(const AdamRule& h, float* w, float* a, float* v, const float* g) { adam_elem(*w, *a, *v, *g, h); }
// a decaying rule on a float4 of a packed tensor: the decay step (optim.h, DecayMomentumRule), every operation rounded on its own,
// then the base rule's own up_step -- decoupled: on the decayed weight; L2: on the gradient that already holds gscale and the decay
// term, with 1 for gscale (1 * g1 is exact)
template <typename Base, typename Rule>
__device__ __forceinline__ void up_step_decay(const Rule& h, f32x4& w, f32x4& a, f32x4& v, f32x4 g) {
#pragma clang fp contract(off)
    // no branch on the mode: both forms are computed and one is selected per component, so the four blocks of a workgroup stay one
    // straight run of arithmetic behind their loads, as in the plain pass (a branch here cost 7 % of the pass: profiles/r17/decay.txt)
    const bool l2 = h.mode != EW_DECAY_DECOUPLED;
    Base b = h;
    b.gscale = l2 ? 1.f : h.gscale;
    const f32x4 dw = h.decay * w, sg = h.gscale * g, g1 = sg + dw, w1 = w - dw;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        w[j] = l2 ? w[j] : w1[j];
        g[j] = l2 ? g1[j] : g[j];
    }
    up_step(b, w, a, v, g);
}
__device__ __forceinline__ void up_step_packed(const DecayMomentumRule& h, f32x4& w, f32x4& a, f32x4& v, const f32x4 g) {
    up_step_decay<MomentumRule>(h, w, a, v, g);
}
__device__ __forceinline__ void up_step_packed(const DecayAdamRule& h, f32x4& w, f32x4& a, f32x4& v, const f32x4 g) {
    up_step_decay<AdamRule>(h, w, a, v, g);
}
}  // namespace
// One workgroup of the packed-tensor path: block (tap, 32-row block rb, group cg of four 32-column blocks) of tensor J, whose gradient is
// `g`. Rule: MomentumRule or AdamRule (the second slot J.v is read in the same batch as w, acc and g), or one of their decaying forms.
template <typename Rule>
__device__ __forceinline__ void update_pack_block(const UpJob& J, float (*tile)[32][33], int tap, int rb, int cg, const Rule& h, const float* g) {
    int seg = 0;
    while (seg + 1 < J.nseg && rb >= J.seg_blk0[seg + 1]) ++seg;
    const int rbs = rb - J.seg_blk0[seg];                // 32-row block inside its segment
    const int r0 = J.seg_r0[seg] + rbs * 32;              // first source row
    const int vr = min(32, J.seg_c[seg] - rbs * 32);      // real rows of the block
    const int r = threadIdx.x >> 3, c4 = (threadIdx.x & 7) * 4;
    // every load of the workgroup's four blocks is issued before the first store: w / acc are read and written through the same (non-restrict)
    // pointers, so a store in front of a later block's loads would order them -- four dependent round trips to memory instead of one
    f32x4 av[4], gv[4], wv[4], vv[4];
    long idx[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int cb = cg * 4 + q, c0 = cb * 32;
        idx[q] = -1;
        av[q] = gv[q] = wv[q] = vv[q] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (cb < J.ncb && r < vr && c0 + c4 < J.R2) {   // (R2 is a multiple of 4: a float4 is inside or outside as a whole)
            const long i = (((long)tap * J.R1 + r0 + r) * J.R2 + c0 + c4) >> 2;
            idx[q] = i;
            av[q] = ((const f32x4*)J.acc)[i];
            if constexpr (Rule::kSecondSlot) vv[q] = ((const f32x4*)J.v)[i];
            gv[q] = ((const f32x4*)g)[i];
            wv[q] = ((const f32x4*)J.w)[i];
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        if (idx[q] >= 0) {
            if constexpr (Rule::kDecay) up_step_packed(h, wv[q], av[q], vv[q], gv[q]);
            else up_step(h, wv[q], av[q], vv[q], gv[q]);
            ((f32x4*)J.acc)[idx[q]] = av[q];
            if constexpr (Rule::kSecondSlot) ((f32x4*)J.v)[idx[q]] = vv[q];
            ((f32x4*)J.w)[idx[q]] = wv[q];
        }
        tile[q][r][c4] = wv[q][0]; tile[q][r][c4 + 1] = wv[q][1]; tile[q][r][c4 + 2] = wv[q][2]; tile[q][r][c4 + 3] = wv[q][3];
    }
    __syncthreads();
    // ---- both packed layouts from LDS: per (column block, destination) 128 pieces of 16 bytes = the 2 tiles of a 32-row pair
    const int npiece = 4 * J.ndest * 128;
    for (int pi = threadIdx.x; pi < npiece; pi += 256) {
        const int p = pi & 127, d = (pi >> 7) % J.ndest, q = pi / (128 * J.ndest);
        const int cb = cg * 4 + q;
        if (cb >= J.ncb) continue;
        const UpDest& D = J.d[d];
        const int tl = p >> 6, lane = p & 63, rho = lane & 15, k0 = 8 * (lane >> 4);
        const int rip = 8 * (rho >> 2) + 4 * tl + (rho & 3);   // row inside the pair of 16-row tiles
        float v[8];
        int chunk, pair;
        if (D.orient == 0) {   // rows from R2 (columns of the block), k from R1 (its rows)
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = tile[q][k0 + j][rip];
            chunk = D.chunk0[seg] + rbs;
            pair = cb;
        } else {               // rows from R1, k from R2
#pragma unroll
            for (int j = 0; j < 8; ++j) v[j] = tile[q][rip][k0 + j];
            chunk = cb;
            pair = rbs;
        }
        const int tapd = D.tapmode == 0 ? tap : (D.tapmode == 1 ? J.ntap - 1 - tap : 0);
        bf16_t* base = D.base[D.orient == 0 ? 0 : (D.tapmode == 2 ? 0 : seg)] + (D.tapmode == 2 ? (long)tap * D.tap_buf_stride : 0);
        const int ntl = D.ntiles[D.orient == 0 || D.tapmode == 2 ? 0 : seg];
        const long e = ((((long)chunk * D.ntap + tapd) * ntl + 2 * pair + tl) << 9) + lane * 8;
        u32x4 o = {pack_bf2(v[0], v[1]), pack_bf2(v[2], v[3]), pack_bf2(v[4], v[5]), pack_bf2(v[6], v[7])};
        *(u32x4*)(base + e) = o;
    }
}
template <typename Rule>
__global__ void __launch_bounds__(256) k_update_pack_many(const UpJob* __restrict__ jobs, int njobs, Rule h) {
    if constexpr (Rule::kDecay) {
        // a decaying rule may come with the record of a clipping rule (below) or without one: the same two lines behind a uniform test
        if (h.state) {
            if (h.state->flags & EW_CLIP_NONFINITE) return;
            h.gscale *= h.state->scale;
        }
    } else if constexpr (Rule::kClip) {
        // a clipping rule is resolved here, once per workgroup, from the record k_grad_norm_final left on this stream: a step whose
        // gradient is not finite is skipped before the first load (weights, slots and packed copies stay as they are, and consistent
        // with each other), any other step runs the arithmetic below unchanged with gscale * scale for gscale (one fp32 multiply)
        if (h.state->flags & EW_CLIP_NONFINITE) return;
        h.gscale *= h.state->scale;
    }
    __shared__ int sj;
    __shared__ float tile[4][32][33];
    if (threadIdx.x < 64) {
        // last job whose block_start <= blockIdx.x = (number of such jobs) - 1 (block_start ascends): every lane tests its share, ONE round
        // trip to L2 instead of the seven dependent ones of a binary search by lane 0 (a third of a workgroup's short life)
        int cnt = 0;
        for (int j = threadIdx.x; j < njobs; j += 64) cnt += jobs[j].block_start <= (int)blockIdx.x ? 1 : 0;
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
        if (threadIdx.x == 0) sj = cnt - 1;
    }
    __syncthreads();
    const UpJob& J = jobs[sj];
    const int b = blockIdx.x - J.block_start;
    if (J.kind == 0) {   // the rule over a contiguous range (the arithmetic of k_momentum / k_adam)
        const long n = J.n, n4 = n >> 2;
        const long i0 = (long)b * (UP_EPB / 4);
        for (int q = 0; q < UP_EPB / 4 / 256; ++q) {
            const long i = i0 + q * 256 + threadIdx.x;
            if (i < n4) {
                f32x4 a = ((f32x4*)J.acc)[i], gv = ((const f32x4*)J.g)[i], wv = ((f32x4*)J.w)[i], vv = {0.f, 0.f, 0.f, 0.f};
                if constexpr (Rule::kSecondSlot) vv = ((f32x4*)J.v)[i];
                up_step(h, wv, a, vv, gv);
                ((f32x4*)J.acc)[i] = a;
                if constexpr (Rule::kSecondSlot) ((f32x4*)J.v)[i] = vv;
                ((f32x4*)J.w)[i] = wv;
            }
        }
        if (b == 0 && threadIdx.x < (n & 3)) {
            const long i = (n4 << 2) + threadIdx.x;
            up_step1(h, J.w + i, J.acc + i, Rule::kSecondSlot ? J.v + i : nullptr, J.g + i);
        }
        return;
    }
    // ---- a packed tensor: workgroup b = (tap, row block rb, group of four column blocks cg)
    const int ncg = (J.ncb + 3) >> 2;
    const int cg = b % ncg, rb = (b / ncg) % J.nrb, tap = b / (ncg * J.nrb);
    update_pack_block(J, tile, tap, rb, cg, h, J.g);
}
int ew_update_job_blocks(const UpJob& j) {
    if (j.kind == 0) return (int)((j.n + UP_EPB - 1) / UP_EPB);
    return j.ntap * j.nrb * ((j.ncb + 3) >> 2);
}
template <typename Rule>
hipError_t ew_update_pack_many(const UpJob* jobs_dev, int njobs, int total_blocks, const Rule& h, hipStream_t st) {
    hipLaunchKernelGGL(k_update_pack_many<Rule>, dim3(total_blocks), dim3(256), 0, st, jobs_dev, njobs, h);
    return hipGetLastError();
}
template hipError_t ew_update_pack_many<MomentumRule>(const UpJob*, int, int, const MomentumRule&, hipStream_t);
template hipError_t ew_update_pack_many<AdamRule>(const UpJob*, int, int, const AdamRule&, hipStream_t);
template hipError_t ew_update_pack_many<ClipMomentumRule>(const UpJob*, int, int, const ClipMomentumRule&, hipStream_t);
template hipError_t ew_update_pack_many<ClipAdamRule>(const UpJob*, int, int, const ClipAdamRule&, hipStream_t);
template hipError_t ew_update_pack_many<DecayMomentumRule>(const UpJob*, int, int, const DecayMomentumRule&, hipStream_t);
template hipError_t ew_update_pack_many<DecayAdamRule>(const UpJob*, int, int, const DecayAdamRule&, hipStream_t);
// ---------------------------------------------------------------------------------------------
// Global norm of the gradient (rsu.h rsu_grad_norm): sum g^2 over g[0, n), read once (4 B per weight, full 128-byte rows), in an order
// that n alone fixes. The caller passes the contiguous [0, n_live) of the flat gradient buffer: the padding floats between its
// variables are zero-initialised and never written, so they add exactly nothing and this is the norm of the live variables (the
// unfused rsu_momentum_step steps the same range on the same grounds).
// Pass 1, workgroup b: float4s [b * EW_GN_EPB / 4, +EW_GN_EPB / 4) of g. A lane issues its 16 loads (float4 q * 256 + lane of the
// share), keeps one fp32 chain per float4 component (16 terms each, q ascending), adds the four chains as (0 + 1) + (2 + 3); the
// n & 3 scalars behind the last float4 go to lanes 0..2 of workgroup 0 as one more term, as in k_update_pack_many. Then a 6-level
// xor tree over the wave and (w0 + w1) + (w2 + w3) over the four waves: ws[b] is the workgroup's sum, ws[nb + b] (as u32) whether one of
// its elements was inf or nan.
// Pass 2, one workgroup: the nb partials in double -- lane t takes t, t + 256, ... ascending, then an 8-level tree in LDS -- and ONE
// thread writes the state record. A second short launch instead of a last-block counter inside pass 1: the counter needs a
// device-scope atomic and a fence per workgroup and a word somebody has to re-zero, and which workgroup comes last is not fixed, so the
// reproducibility of the result would rest on the finisher re-reading every partial in a fixed order anyway -- which is this launch.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_grad_norm_partial(const float* __restrict__ g, long n, float* __restrict__ ws, int nb) {
    const long n4 = n >> 2;
    const long i0 = (long)blockIdx.x * (EW_GN_EPB / 4) + threadIdx.x;
    f32x4 v[EW_GN_EPB / 4 / 256];
#pragma unroll
    for (int q = 0; q < EW_GN_EPB / 4 / 256; ++q) {
        const long i = i0 + q * 256;
        v[q] = i < n4 ? ((const f32x4*)g)[i] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    unsigned bad = 0u;   // an exponent of all ones: inf or nan
#pragma unroll
    for (int q = 0; q < EW_GN_EPB / 4 / 256; ++q) {
        s += v[q] * v[q];
#pragma unroll
        for (int j = 0; j < 4; ++j) bad |= (__float_as_uint(v[q][j]) & 0x7f800000u) == 0x7f800000u ? 1u : 0u;
    }
    float t = (s[0] + s[1]) + (s[2] + s[3]);
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const float x = g[(n4 << 2) + threadIdx.x];
        t += x * x;
        bad |= (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u ? 1u : 0u;
    }
    for (int o = 32; o > 0; o >>= 1) {
        t += __shfl_xor(t, o);
        bad |= __shfl_xor(bad, o);
    }
    __shared__ float ssum[4];
    __shared__ unsigned sbad[4];
    if ((threadIdx.x & 63) == 0) {
        ssum[threadIdx.x >> 6] = t;
        sbad[threadIdx.x >> 6] = bad;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        ws[blockIdx.x] = (ssum[0] + ssum[1]) + (ssum[2] + ssum[3]);
        ((unsigned*)ws)[nb + blockIdx.x] = sbad[0] | sbad[1] | sbad[2] | sbad[3];
    }
}
__global__ void __launch_bounds__(256) k_grad_norm_final(const float* __restrict__ ws, int nb, float max_norm, ClipState* __restrict__ state) {
    __shared__ double dsum[256];
    __shared__ unsigned dbad[256];
    double t = 0.0;
    unsigned bad = 0u;
    for (int b = threadIdx.x; b < nb; b += 256) {
        t += (double)ws[b];
        bad |= ((const unsigned*)ws)[nb + b];
    }
    dsum[threadIdx.x] = t;
    dbad[threadIdx.x] = bad;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            dsum[threadIdx.x] += dsum[threadIdx.x + o];
            dbad[threadIdx.x] |= dbad[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {   // the single writer of the record
        const float sumsq = (float)dsum[0];   // (a double sum above FLT_MAX rounds to inf: an overflow counts as not finite)
        const float norm = (float)sqrt((double)sumsq);
        const bool nonfinite = dbad[0] != 0u || (__float_as_uint(sumsq) & 0x7f800000u) == 0x7f800000u;
        const bool clipped = !nonfinite && norm > max_norm;
        ClipState r = *state;
        r.sumsq = sumsq;
        r.norm = norm;
        r.scale = nonfinite ? 0.f : (clipped ? (float)((double)max_norm / (double)norm) : 1.f);
        r.flags = (clipped ? EW_CLIP_CLIPPED : 0u) | (nonfinite ? EW_CLIP_NONFINITE : 0u);
        r.steps += 1u;
        r.clipped_steps += clipped ? 1u : 0u;
        r.skipped_steps += nonfinite ? 1u : 0u;
        r.pad = 0u;
        *state = r;
    }
}
int ew_grad_norm_blocks(long n) {
    const long nb = ((n >> 2) + EW_GN_EPB / 4 - 1) / (EW_GN_EPB / 4);
    return (int)(nb < 1 ? 1 : nb);
}
hipError_t ew_grad_norm(const float* g, long n, float max_norm, float* ws, ClipState* state, hipStream_t st) {
    const int nb = ew_grad_norm_blocks(n);
    hipLaunchKernelGGL(k_grad_norm_partial, dim3(nb), dim3(256), 0, st, g, n, ws, nb);
    hipLaunchKernelGGL(k_grad_norm_final, dim3(1), dim3(256), 0, st, ws, nb, max_norm, state);
    return hipGetLastError();
}
// ---------------------------------------------------------------------------------------------
// Exponential moving average of the weights (rsu.h rsu_ema_step): ema -= (ema - w) * one_minus_decay over [0, n), TensorFlow's
// assign_moving_average in float32, two roundings per step besides the subtraction's (no contraction: an FMA would move the last bit
// against a float32 restatement). Reads ema and w once, writes ema: 12 B per weight, full 128-byte rows. The grid is
// k_grad_norm_partial's, cdiv(n / 4, EW_EMA_EPB / 4) (at least 1): workgroup b owns float4s [b * EW_EMA_EPB / 4, +EW_EMA_EPB / 4), a
// lane float4 q * 256 + lane of that share, and issues its 2 x EW_EMA_EPB / 1024 loads before its first store (ema is read and written
// through one pointer: a store in front of a later load would order them). The n & 3 scalars behind the last float4 go to lanes 0..2
// of workgroup 0. `state`, when not NULL, is the record k_grad_norm_final left on this stream: with EW_CLIP_NONFINITE set the update
// pass skipped its step, and every workgroup here returns before its first load as well -- the averages of a skipped step do not move.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float ema_elem(float e, float w, float omd) {
#pragma clang fp contract(off)
    return e - (e - w) * omd;
}
// one lane's part of a workgroup's share; FULL: the whole share lies inside [0, n4), no lane tests anything (every workgroup but the last)
template <bool FULL>
__device__ __forceinline__ void ema_share(float* ema, const float* __restrict__ w, long i0, long n4, float omd) {
    constexpr int NQ = EW_EMA_EPB / 4 / 256;
    f32x4 ev[NQ], wv[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const long i = i0 + q * 256;
        const bool in = FULL || i < n4;
        ev[q] = in ? ((const f32x4*)ema)[i] : f32x4{0.f, 0.f, 0.f, 0.f};
        wv[q] = in ? ((const f32x4*)w)[i] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const long i = i0 + q * 256;
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = ema_elem(ev[q][j], wv[q][j], omd);
        if (FULL || i < n4) ((f32x4*)ema)[i] = o;
    }
}
__global__ void __launch_bounds__(256) k_ema(float* ema, const float* __restrict__ w, long n, float omd, const ClipState* __restrict__ state) {
    if (state && (state->flags & EW_CLIP_NONFINITE)) return;
    const long n4 = n >> 2;
    const long b0 = (long)blockIdx.x * (EW_EMA_EPB / 4);
    if (b0 + EW_EMA_EPB / 4 <= n4) ema_share<true>(ema, w, b0 + threadIdx.x, n4, omd);
    else ema_share<false>(ema, w, b0 + threadIdx.x, n4, omd);
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const long i = (n4 << 2) + threadIdx.x;
        ema[i] = ema_elem(ema[i], w[i], omd);
    }
}
int ew_ema_blocks(long n) {
    const long nb = ((n >> 2) + EW_EMA_EPB / 4 - 1) / (EW_EMA_EPB / 4);
    return (int)(nb < 1 ? 1 : nb);
}
hipError_t ew_ema(float* ema, const float* w, long n, float one_minus_decay, const ClipState* state, hipStream_t st) {
    hipLaunchKernelGGL(k_ema, dim3(ew_ema_blocks(n)), dim3(256), 0, st, ema, w, n, one_minus_decay, state);
    return hipGetLastError();
}
// ---------------------------------------------------------------------------------------------
// Gradient accumulation (rsu.h rsu_grad_accumulate): dst[i] = src[i] (ASSIGN) or dst[i] + src[i] over [0, n), float32, one rounding
// per element. The shape of k_ema: the grid cdiv(n / 4, EW_ACC_EPB / 4) (at least 1) depends on n alone, workgroup b owns float4s
// [b * EW_ACC_EPB / 4, +EW_ACC_EPB / 4), a lane float4 q * 256 + lane of that share, and a lane issues all its loads before its first
// store (dst is read and written through one pointer). ASSIGN never reads dst -- whatever it held, a nan included, is forgotten -- and
// moves 8 B per weight instead of 12. The n & 3 scalars behind the last float4 go to lanes 0..2 of workgroup 0. inf and nan pass by the
// IEEE rules; nothing is filtered.
// ---------------------------------------------------------------------------------------------
// one lane's part of a workgroup's share; FULL: the whole share lies inside [0, n4), no lane tests anything (every workgroup but the last)
template <bool FULL, bool ASSIGN>
__device__ __forceinline__ void acc_share(float* dst, const float* __restrict__ src, long i0, long n4) {
    constexpr int NQ = EW_ACC_EPB / 4 / 256;
    f32x4 dv[NQ], sv[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const long i = i0 + q * 256;
        const bool in = FULL || i < n4;
        if (!ASSIGN) dv[q] = in ? ((const f32x4*)dst)[i] : f32x4{0.f, 0.f, 0.f, 0.f};
        sv[q] = in ? ((const f32x4*)src)[i] : f32x4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        const long i = i0 + q * 256;
        f32x4 o = sv[q];
        if (!ASSIGN) {
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = dv[q][j] + sv[q][j];
        }
        if (FULL || i < n4) ((f32x4*)dst)[i] = o;
    }
}
template <bool ASSIGN>
__global__ void __launch_bounds__(256) k_grad_accumulate(float* dst, const float* __restrict__ src, long n) {
    const long n4 = n >> 2;
    const long b0 = (long)blockIdx.x * (EW_ACC_EPB / 4);
    if (b0 + EW_ACC_EPB / 4 <= n4) acc_share<true, ASSIGN>(dst, src, b0 + threadIdx.x, n4);
    else acc_share<false, ASSIGN>(dst, src, b0 + threadIdx.x, n4);
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
        const long i = (n4 << 2) + threadIdx.x;
        dst[i] = ASSIGN ? src[i] : dst[i] + src[i];
    }
}
int ew_grad_accumulate_blocks(long n) {
    const long nb = ((n >> 2) + EW_ACC_EPB / 4 - 1) / (EW_ACC_EPB / 4);
    return (int)(nb < 1 ? 1 : nb);
}
hipError_t ew_grad_accumulate(float* dst, const float* src, long n, bool assign, hipStream_t st) {
    const dim3 grid(ew_grad_accumulate_blocks(n));
    if (assign) hipLaunchKernelGGL(k_grad_accumulate<true>, grid, dim3(256), 0, st, dst, src, n);
    else hipLaunchKernelGGL(k_grad_accumulate<false>, grid, dim3(256), 0, st, dst, src, n);
    return hipGetLastError();
}
hipError_t ew_momentum(float* w, float* acc, const float* g, float lr, float mu, float gscale, long n, hipStream_t st) {
    hipLaunchKernelGGL(k_momentum, dim3(grid_for((n + 3) / 4, 256)), dim3(256), 0, st, w, acc, g, lr, mu, gscale, n);
    return hipGetLastError();
}
hipError_t ew_adam(float* w, float* m, float* v, const float* g, const AdamRule& h, long n, hipStream_t st) {
    hipLaunchKernelGGL(k_adam, dim3(grid_for((n + 3) / 4, 256)), dim3(256), 0, st, w, m, v, g, h, n);
    return hipGetLastError();
}
