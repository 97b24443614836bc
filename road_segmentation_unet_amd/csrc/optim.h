// Launch prototypes, rule structs and constants of the optimizer step's kernels (optim.hip).
#pragma once
#include "rsu_common.h"

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
struct AdamRule {       // TensorFlow 1.x ApplyAdam with alpha = lr_t * sqrt(1 - beta2^t) / (1 - beta1^t) from the host (optim.hip, adam_elem)
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
// the launch of k_update_pack_many<Rule>: instantiated in optim.hip for the six rules above
template <typename Rule>
hipError_t ew_update_pack_many(const UpJob* jobs_dev, int njobs, int total_blocks, const Rule& h, hipStream_t st);
