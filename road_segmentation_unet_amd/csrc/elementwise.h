// Launch prototypes of the bandwidth-bound kernels (elementwise.hip).
#pragma once
#include "rsu_common.h"

struct PackParams {
    int nchunks, ntap, ntiles;  // packed dims: [nchunks][ntap][ntiles][64][8]
    int rows;                   // real output rows (channels)
    int nseg, seg_c[3];         // K segments (concat sources), real channel counts
    long s_tap, s_row, s_k;     // source strides (elements)
    int flip;                   // read source tap (ntap-1-tap)
};

hipError_t ew_color_adjust(const float* x, const float* w, const float* b, void* out16, long npix, float keep, unsigned key, hipStream_t st);
hipError_t ew_scale_bf16(void* x, long n, float s, hipStream_t st);
hipError_t ew_dropout(const void* x, void* y, long n, float keep, unsigned key, hipStream_t st);
hipError_t ew_scatter_first_grads(const float* tmp, float* dw1, float* gxc, int Cout, hipStream_t st);
hipError_t ew_maxpool_fwd(const void* x, void* y, void* code, int N, int H, int W, int C, float keep, unsigned key, hipStream_t st);
hipError_t ew_pool_skip_relu_bwd(const void* yact, const void* code, const void* dpool, const void* dskip, void* dz, int N, int H, int W, int C, int Hs, int Ws,
                                 float keep, unsigned key, hipStream_t st);
int ew_colsum_blocks(long npix, int C);
hipError_t ew_colsum(const void* dz, float* db, float* ws, long npix, int C, hipStream_t st);
// out2 (optional): n2 more float4 items behind the taps of every slab, reduced into out2 by the same launch
hipError_t ew_reduce_slabs(const float* slab, float* out, float* out2, int n2, int nsplit, long slab_elems, int ntap, int CsOut, int cs_off, int cs_cnt,
                           int CfOut, hipStream_t st);
// grouped form: one launch reduces the slabs of several weight-gradient jobs (device-resident job table)
struct ReduceJob {
    const float* slab; float* out; float* out2;
    long slab_elems;
    int n2, nsplit, ntap, CsOut, cs_off, cs_cnt, CfOut;
    int block_begin, wide, pad_;
};
int ew_reduce_job_blocks(ReduceJob& j);   // sets j.wide, returns the workgroups the job needs
hipError_t ew_reduce_slabs_many(const ReduceJob* jobs_dev, int njobs, int total_blocks, hipStream_t st);
int ew_head_blocks(long npix, int C);
hipError_t ew_head(bool train, const void* act, const float* w, const float* b, const int64_t* labels, float* prob, float* logits, void* dact, float* dw,
                   float* db, float* loss_sum, float* ws, long npix, int C, float inv_count, hipStream_t st);
// the weighted training head and pass B of the soft-Dice head (rsu.h rsu_head_fwd_bwd_w, rsu_head_fwd_bwd_dice): same grid, ws of
// ew_head_blocks() * (2 C + 4) floats; dice_sums == nullptr: no Dice term (dice_scale and smooth are not read)
hipError_t ew_head_loss(const void* act, const float* w, const float* b, const int64_t* labels, const float* class_w, const float* pixel_w,
                        const float* dice_sums, float dice_scale, float smooth, float* prob, void* dact, float* dw, float* db, float* loss_sum,
                        float* weight_sum, float* ws, long npix, int C, float inv_count, hipStream_t st);
// pass A of the soft-Dice head (rsu.h rsu_head_dice_sums): same grid, ws of ew_head_blocks() * 3 floats
hipError_t ew_head_dice_sums(const void* act, const float* w, const float* b, const int64_t* labels, const float* pixel_w, float* prob,
                             float* dice_sums, float* ws, long npix, int C, hipStream_t st);
// the evaluation head (rsu.h rsu_head_eval): same grid, forward only; ws of ew_head_eval_ws_floats() floats (5 partial sums and one
// 2 x EW_EVAL_BINS row of u32 counters per workgroup). EW_EVAL_BINS is rsu.h's RSU_EVAL_BINS.
constexpr int EW_EVAL_BINS = 256;
constexpr int EW_EVAL_SLICES = 8;   // k_head_eval_final: workgroups per 64-bin group (= adds per address of hist per call)
size_t ew_head_eval_ws_floats(long npix, int C);
hipError_t ew_head_eval(const void* act, const float* w, const float* b, const int64_t* labels, const float* class_w, const float* pixel_w,
                        float* prob, float* sums, unsigned long long* hist, float* ws, long npix, int C, hipStream_t st);
hipError_t ew_color_adjust_bwd(const float* gx, const float* w1, float* dW0, float* db0, int Cout, float scale, int accumulate, hipStream_t st);
hipError_t ew_momentum(float* w, float* acc, const float* g, float lr, float mu, float gscale, long n, hipStream_t st);
// the update rules of the optimizer passes (template argument of k_update_pack_many): their scalars, passed by value to the kernels.
// kSecondSlot: the rule keeps a second fp32 slot per weight (UpJob::v)
// kClip: the rule takes a factor of gscale, and the decision to step at all, from a ClipState in device memory (k_update_pack_many's head)
// kDecay: the rule decays the weights of the packed tensors (DecayMomentumRule / DecayAdamRule below)
struct MomentumRule {   // acc = mu * acc + gscale * g; w -= lr * acc
    float lr, mu, gscale;
    static constexpr bool kSecondSlot = false;
    static constexpr bool kClip = false;
    static constexpr bool kDecay = false;
};
struct AdamRule {       // TensorFlow 1.x ApplyAdam with alpha = lr_t * sqrt(1 - beta2^t) / (1 - beta1^t) from the host (elementwise.hip, adam_elem)
    float alpha, beta1, beta2, epsilon, gscale;
    static constexpr bool kSecondSlot = true;
    static constexpr bool kClip = false;
    static constexpr bool kDecay = false;
};
// Global-norm gradient clipping (rsu.h rsu_grad_norm): the 32-byte state record, rsu.h's layout field by field. One thread of
// k_grad_norm_final writes it; the clipping rules below read scale and flags from it, so the host never has to.
struct ClipState {
    float sumsq, norm, scale;
    unsigned flags;                                 // EW_CLIP_CLIPPED | EW_CLIP_NONFINITE
    unsigned steps, clipped_steps, skipped_steps;   // accumulate over the calls
    unsigned pad;
};
constexpr unsigned EW_CLIP_CLIPPED = 1u, EW_CLIP_NONFINITE = 2u;
// the same two rules with gscale * state->scale for gscale; a workgroup returns before its first load when state->flags has EW_CLIP_NONFINITE
struct ClipMomentumRule : MomentumRule {
    const ClipState* state;
    static constexpr bool kClip = true;
};
struct ClipAdamRule : AdamRule {
    const ClipState* state;
    static constexpr bool kClip = true;
};
// Weight decay inside the update pass (rsu_optim.h rsu_update_table_run_decay / _adam_decay): the two rules with a decay step on every
// element of a PACKED tensor (UpJob::kind != 0); plain ranges run the plain rule. mode (uniform; both forms are computed and one selected):
//   EW_DECAY_DECOUPLED  w1 = w - (decay * w), then the rule on (w1, slots, g)
//   EW_DECAY_L2         g1 = (gscale * g) + (decay * w), then the rule with g1 for gscale * g
// each operation one float32 rounding (no contraction). state: nullptr, or the record of ew_grad_norm, read as a clipping rule reads it.
constexpr int EW_DECAY_L2 = 0, EW_DECAY_DECOUPLED = 1;
struct DecayMomentumRule : MomentumRule {
    const ClipState* state;   // (first: the layout of the clipping rules, base + pointer, which the compiler keeps in registers)
    float decay;
    int mode;
    static constexpr bool kDecay = true;
};
struct DecayAdamRule : AdamRule {
    const ClipState* state;   // (first: the layout of the clipping rules, base + pointer, which the compiler keeps in registers)
    float decay;
    int mode;
    static constexpr bool kDecay = true;
};
// floats of g per workgroup of the norm's pass 1: 256 lanes x 16 float4. The grid, cdiv(n / 4, EW_GN_EPB / 4) (at least 1), depends on
// n alone -- not on the CU budget, the device or the autotuner -- so the order of every sum, and with it the bits of the norm, do too.
constexpr int EW_GN_EPB = 16384;
int ew_grad_norm_blocks(long n);
hipError_t ew_grad_norm(const float* g, long n, float max_norm, float* ws, ClipState* state, hipStream_t st);
// Moving average of the weights (rsu.h rsu_ema_step): floats per workgroup, 256 lanes x 8 float4 of each of the two arrays. The grid,
// cdiv(n / 4, EW_EMA_EPB / 4) (at least 1), depends on n alone. state: nullptr, or the record of ew_grad_norm (a skipped step skips here too)
constexpr int EW_EMA_EPB = 8192;
int ew_ema_blocks(long n);
hipError_t ew_ema(float* ema, const float* w, long n, float one_minus_decay, const ClipState* state, hipStream_t st);
// Gradient accumulation (rsu.h rsu_grad_accumulate): floats per workgroup, 256 lanes x 8 float4 of src (and, when adding, of dst). The
// grid, cdiv(n / 4, EW_ACC_EPB / 4) (at least 1), depends on n alone. assign: dst = src and dst is never read; else dst += src
constexpr int EW_ACC_EPB = 8192;
int ew_grad_accumulate_blocks(long n);
hipError_t ew_grad_accumulate(float* dst, const float* src, long n, bool assign, hipStream_t st);
hipError_t ew_adam(float* w, float* m, float* v, const float* g, const AdamRule& h, long n, hipStream_t st);
hipError_t ew_pack(const float* src, void* dst, const PackParams& pp, hipStream_t st);
struct PackJob { PackParams pp; const float* src; bf16_t* dst; int block_start; int pad_; };
hipError_t ew_pack_many(const PackJob* jobs_dev, int njobs, int total_blocks, hipStream_t st);
int ew_pack_blocks(const PackParams& pp);
// Momentum + re-pack in one pass (k_update_pack_many): one destination of a tensor's packed copies
struct UpDest {
    bf16_t* base[3];        // orientation B with tapmode 0/1: one buffer per segment of R1 (concat source); else base[0]
    long tap_buf_stride;    // tapmode 2 (one single-tap matrix per source tap): elements between the matrices
    int orient;             // 0: rows from R2, k from R1 (segmented, 32-padded); 1: rows from R1 (of one segment), k from R2
    int ntap, tapmode;      // taps of the packed layout; 0 same tap, 1 flipped, 2 tap 0 of the tap's own matrix
    int ntiles[3];          // 16-row tiles per (chunk, tap) of the packed layout (orientation 1: of each segment's buffer)
    int chunk0[3];          // orientation 0: first 32-k chunk of each R1 segment
};
struct UpJob {
    float* w; float* acc; const float* g;
    long n;                 // kind 0: floats of the range
    int kind;               // 0 plain Momentum range, 1 packed tensor
    int ntap, R1, R2;       // source [ntap][R1][R2], R2 contiguous
    int nseg, seg_c[3], seg_r0[3], seg_blk0[3];   // R1 segments: real rows, first row, first 32-row block
    int nrb, ncb;           // 32-blocks along R1 (all segments) and along R2
    int ndest;
    UpDest d[2];
    int block_start, pad_;
    float* v;               // the second slot of a rule that keeps one (Adam: v; `acc` is its m), else unused
};
int ew_update_job_blocks(const UpJob& j);
hipError_t ew_update_pack_many(const UpJob* jobs_dev, int njobs, int total_blocks, float lr, float mu, float gscale, hipStream_t st);
hipError_t ew_update_pack_many_adam(const UpJob* jobs_dev, int njobs, int total_blocks, const AdamRule& h, hipStream_t st);
hipError_t ew_update_pack_many_clip(const UpJob* jobs_dev, int njobs, int total_blocks, const ClipMomentumRule& h, hipStream_t st);
hipError_t ew_update_pack_many_adam_clip(const UpJob* jobs_dev, int njobs, int total_blocks, const ClipAdamRule& h, hipStream_t st);
hipError_t ew_update_pack_many_decay(const UpJob* jobs_dev, int njobs, int total_blocks, const DecayMomentumRule& h, hipStream_t st);
hipError_t ew_update_pack_many_adam_decay(const UpJob* jobs_dev, int njobs, int total_blocks, const DecayAdamRule& h, hipStream_t st);
hipError_t ew_extract_tiles(const float* imgs, float* tiles, int H, int S, int P, int stride, int pps, long t0, long ntiles, hipStream_t st);
hipError_t ew_overlap_add(const float* prob, float* acc, float* hits, int nimg, int H, int P, int stride, int pps, long t0, long ntiles, hipStream_t st);
hipError_t ew_overlap_finish(const float* acc, const float* hits, float* out, long n, hipStream_t st);
void ew_tile_grid(int H, int W, int P, int stride, int* ny, int* nx);
hipError_t ew_extract_tiles_rect(const float* imgs, float* tiles, int H, int W, int S, int P, int stride, long t0, long ntiles, hipStream_t st);
hipError_t ew_overlap_add_rect(const float* prob, float* acc, float* hits, int nimg, int H, int W, int P, int stride, long t0, long ntiles,
                               hipStream_t st);
hipError_t ew_block_label_rect(const float* mask, float* out, int nimg, int H, int W, int ps, float thr, hipStream_t st);
hipError_t ew_block_label(const float* mask, float* out, int64_t* labels, int nimg, int S, int ps, float thr, int mode, hipStream_t st);
hipError_t ew_confusion(const int64_t* pred, const int64_t* truth, long n, unsigned long long* counts, hipStream_t st);
