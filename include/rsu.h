/*
 * rsu.h -- C ABI of the MI355X-native U-Net hot path (librsu_hip.so).
 *
 * The reference (aschneuw/road-segmentation-unet) is pure Python over TensorFlow 1.4; it has no
 * FFI of its own. The operator boundary this library replaces is the set of TF op kernels that
 * /root/reference/src/unet.py:12-97 and src/tf_aerial_images.py:103-122,147-149 instantiate, plus
 * the numpy tiler of src/images.py. Every entry point below cites the reference call site it
 * stands in for. INTEGRATION.md shows the ctypes binding a maintainer of the reference would add.
 *
 * Conventions
 *   - plain C: device pointers + sizes, no torch / C++ types. `stream` is a hipStream_t passed
 *     as void* (NULL = the default stream). All calls are asynchronous on that stream and
 *     re-entrant per stream. Every MFMA launch takes the compute units it may plan for as its own `ncu` argument; nothing has
 *     to be set between launches. Process-wide state (advisory, none of it changes a result): the DEFAULT budget behind ncu = 0
 *     (rsu_set_cu_budget), the tile-shape tuning mode and its table of measured choices (rsu_set_autotune: launches look shapes
 *     up and never measure unless the host switches to RSU_TUNE_MEASURE for an explicit tuning pass), one page of zeros per device.
 *   - devices: one process drives one GPU (torch.distributed, one rank per device). The HIP current device must be the device
 *     the stream and the pointers belong to (the Python host calls torch.cuda.set_device); tensors stay below 2 GiB each
 *     (RSU_E2BIG otherwise: split the batch).
 *   - the 2-GiB rule: EVERY batch-taking entry point -- the MFMA launches and the VALU ones (colour adjust, dropout, pools, gradient
 *     junction, heads, bias gradient) alike -- returns RSU_E2BIG, before anything is launched or written, when one of the tensors it is
 *     handed has 0x7ffffff0 bytes or more; below that every entry is exact (tests/test_gpu_large_tensors.py runs each one image short of
 *     the limit against the oracle, tests/test_large_limits_host.py holds each to its refusal one image past it). Which tensor that is,
 *     is noted at each entry as "limit:". The decision for the VALU entries is REFUSE, not "exact beyond 2 GiB": their kernels use 64-bit
 *     addresses, but their dropout counters are 32-bit element indices and k_pool_skip_relu_bwd_code forms its pooled element index and
 *     its row count N * (H / 2) in int; no caller needs more, since every conv around these launches refuses such tensors.
 *   - activations: NHWC, bfloat16 ("bf16", the storage type of the fast path), raw uint16 bits.
 *     Channel counts of bf16 tensors must be multiples of 8 (16-byte pieces).
 *   - parameters / gradients / optimizer state: float32 in the reference's own layouts: conv
 *     kernels HWIO [kh][kw][Cin][Cout] (tf.layers.conv2d), transposed-conv kernels
 *     [kh][kw][Cout][Cin] (tf.layers.conv2d_transpose).
 *   - MFMA kernels read bf16 copies of the weights in "fragment order" produced by the
 *     rsu_pack_* calls (re-pack after every optimizer step).
 *   - return value: 0 on success, negative errno-style code otherwise (never throws).
 *
 * Memory contract
 *   An entry point reads and writes only [ptr, ptr + size) of the tensors it is given, with the sizes this header states for them (of a
 *   cropped rsu_src_t: the whole [N][H][W][C] tensor, its window included), and only [0, advertised) of a workspace, `advertised` being
 *   what the entry's rsu_*_ws_floats / rsu_*_ws_bytes function returns; a packed weight buffer has exactly rsu_packed_bytes /
 *   rsu_packed_first_bytes bytes. It writes nothing to its inputs, and its results do not depend on whatever lies around any of these
 *   ranges: a caller may place its buffers back to back. The kernels' buffer descriptors do not bound anything: the
 *   contract rests on the kernels' own predicates, and tests/test_gpu_fenced.py holds every launching entry point to it inside an arena
 *   whose every byte outside the payloads is a NaN pattern.
 *   Alignment: every launching entry point (and every call that stores a device pointer in a table for a later launch) states at its
 *   prototype, as "align (entry): argument bytes, ...", the alignment of each pointer argument: the widest single access or atomic the
 *   kernels make through it (16 for the 16-byte pieces of a bf16 tensor or of packed weights and for float4 passes, 8 for 64-bit labels,
 *   keys, plane words and counters, 4 for tensors read float by float), for a workspace the largest need of anything carved out of it;
 *   "host" marks host memory that is read before the call returns, "byte" a tensor of bytes. A key "p.field" or "p[]" is a device pointer
 *   inside the host struct or array p. A non-NULL pointer that is no multiple of its number is RSU_EINVAL, before anything is launched or
 *   written; NULL keeps the meaning it has at the entry; at the stated alignment -- and at no larger one -- every entry is exact:
 *   tests/test_align_limits_host.py holds each entry to its refusal, tests/test_gpu_aligned_min.py runs each inside the arena with every
 *   buffer at 256 k + its number. Nothing else is assumed: a buffer that follows another back to back needs only its own alignment.
 *   Workspaces: a `ws` or `kws` argument, in this header and in the family headers, need not be cleared and holds nothing between
 *   calls -- the launches of ONE call initialise every word of it that they read, and no result depends on what it held before, be it
 *   zeros, ones, or what another entry, another layer or another batch left there (one buffer may serve them all in turn, as UNet.ws
 *   does). The exceptions are named where they occur: rsu_cldice_bwd reads what rsu_cldice_fwd wrote (rsu_cldice.h), and a group's ws
 *   belongs to the group from rsu_wgrad_group_run to the end of its stream work. Sums that travel between two calls do so in arguments
 *   of their own (dice_sums, sums, state), never in a workspace; an accumulator the caller zeroes (loss_sum, acc, sums, hist) is no
 *   workspace. tests/test_gpu_ws_history.py runs every entry that takes a workspace with it zeroed, filled with 0xFF and filled with the
 *   rolled leftover of an earlier call, and asks for the same bytes in every output each time.
 */
#ifndef RSU_H_
#define RSU_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RSU_OK 0
#define RSU_EINVAL (-22)  /* bad geometry / unsupported shape (the reference raises AssertionError) */
#define RSU_ENOMEM (-12)  /* workspace too small */
#define RSU_EHIP (-5)     /* a HIP runtime call failed; see rsu_last_hip_error() */
#define RSU_E2BIG (-7)    /* a tensor of this call reaches 2 GiB (32-bit byte offsets inside the kernels): use a smaller batch */

typedef void* rsu_stream_t; /* hipStream_t */

/* One input of a (virtually concatenated) convolution: a window of an NHWC bf16 tensor.
 * unet.py:70-85 crops the skip tensor(s) to the up-conv size and concatenates [skip,(dil skip),up]
 * on the channel axis; this library never materialises that tensor: the conv reads up to three
 * sources, each with its own crop offset (oy, ox) = ((H - h) / 2, (W - w) / 2). */
typedef struct {
    const void* ptr; /* bf16 [N][H][W][C] */
    int H, W, C;
    int oy, ox; /* origin of the window inside the tensor */
} rsu_src_t;

/* ---- library / device ------------------------------------------------------------------- */
const char* rsu_version(void);
int rsu_last_hip_error(void);
/* Compute units a persistent MFMA launch plans for (one workgroup each). New here (the reference is single-device). Every
 * MFMA entry point below takes it as its `ncu` argument, 32..256 (256 = the whole MI355X); ncu = 0 selects the process default
 * set here (256 unless changed). A data-parallel host leaves some CUs to the RCCL channel workgroups of an overlapped gradient
 * all-reduce; the Python host (unet.py, RSU_SPLIT_CHIP) gives the backward-data launches of its main stream and the
 * weight-gradient launches of its side stream disjoint shares of the chip, so that one kernel of each kind is resident at a
 * time. For the weight gradients ncu sets the number of partial sums per output tile: it changes their summation order
 * (results agree to fp32 rounding); for every other launch it only changes speed. */
int rsu_set_cu_budget(int ncu);
int rsu_get_cu_budget(void);
/* Tile shapes of the conv launches by measurement. All shapes give bit-identical results; the mode only moves time.
 *   RSU_TUNE_OFF      the cost model decides (RSU_AUTOTUNE=0 in the environment forces this);
 *   RSU_TUNE_LOOKUP   (default) a launch uses the measured shape of its (geometry, flags, ncu) if the table holds one, else the
 *                     model's; it never measures, so the launch entry points never synchronise the device;
 *   RSU_TUNE_MEASURE  a launch whose key is missing times every admissible shape on an idle device (synchronises it) and keeps
 *                     the fastest if it beats the model's choice by 3 %. The host switches this on around ONE explicit, untimed
 *                     pass over its network (UNet.tune) -- under data parallelism before any collective is in flight.
 * rsu_autotune_entries: geometries measured so far. */
#define RSU_TUNE_OFF 0
#define RSU_TUNE_LOOKUP 1
#define RSU_TUNE_MEASURE 2
int rsu_set_autotune(int mode);
int rsu_get_autotune(void);
int rsu_autotune_entries(void);
/* The table of measured choices as rows of 17 ints (opaque key words + choice): export after a run, import before another (a
 * profiling run then issues no timing launches). export returns the number of entries (rows may be NULL to count); import
 * returns the number of rows it took: rows naming a tile shape or kernel generation this build does not have are skipped (the
 * host also stamps its file with the library's hash, bench.py). */
int rsu_autotune_export(int* rows, int capacity);
int rsu_autotune_import(const int* rows, int nrows);
/* unet.py:100-115 input_size_needed(output_size, num_layers). RSU_EINVAL where the reference asserts. */
int rsu_input_size_needed(int output_size, int num_layers, int* input_size);

/* ---- weight packing (float32 reference layout -> bf16 MFMA fragment order) -------------- */
/* Bytes of a packed buffer: taps * sum_i roundup(seg_c[i],32) * roundup(rows,128) * 2. The rsu_pack_* calls and rsu_pack_table_run write
 * every byte of it, the zero padding of the fragment order included: the buffer needs no initialisation. */
size_t rsu_packed_bytes(int taps, int rows, const int* seg_c, int nseg);
/* conv forward (unet.py:34-45,88-91): A[tap][co][ci]; seg_c = channel count of each concat source */
/* align (rsu_pack_conv_fwd): w_hwio 4, packed 2, seg_c host. */
int rsu_pack_conv_fwd(const float* w_hwio, void* packed, int k, int Cin, int Cout, const int* seg_c, int nseg,
                      rsu_stream_t stream);
/* conv backward-data (Conv2DBackpropInput): A[flipped tap][ci][co] for the input channels
 * [ci_off, ci_off+ci_cnt) of a kernel with Cin_total inputs (one pack per concat source) */
/* align (rsu_pack_conv_bwd): w_hwio 4, packed 2. */
int rsu_pack_conv_bwd(const float* w_hwio, void* packed, int k, int Cin_total, int ci_off, int ci_cnt, int Cout,
                      rsu_stream_t stream);
/* transposed conv forward (unet.py:67-68): four 1x1 matrices A[a*2+b][co][ci] */
/* align (rsu_pack_convT_fwd): k_hwoi 4, packed 2. */
int rsu_pack_convT_fwd(const float* k_hwoi, void* packed, int Cin, int Cout, rsu_stream_t stream);
/* transposed conv backward-data: A[a*2+b][ci][co] */
/* align (rsu_pack_convT_bwd): k_hwoi 4, packed 2. */
int rsu_pack_convT_bwd(const float* k_hwoi, void* packed, int Cin, int Cout, rsu_stream_t stream);

/* Batched packing: every weight tensor of the network re-packed by ONE kernel launch (the per-tensor calls above cost a
 * launch each, ~64 per optimizer step). Fill a host table with rsu_pack_table_add (same arguments as the per-tensor
 * calls, selected by `kind`), copy it to the device once (the pointers are static), then call rsu_pack_table_run after
 * every optimizer step. Returns the number of table entries used by the tensor (4 for RSU_PACK_CONVT_FWD, else 1). */
#define RSU_PACK_CONV_FWD 0
#define RSU_PACK_CONV_BWD 1
#define RSU_PACK_CONVT_FWD 2
#define RSU_PACK_CONVT_BWD 3
#define RSU_PACK_CONV_FIRST 4
size_t rsu_pack_table_entry_bytes(void);
/* align (rsu_pack_table_add): host_table host, w 4, packed 16, seg_c host. */
int rsu_pack_table_add(void* host_table, int index, int kind, const float* w, void* packed, int k, int Cin_total, int ci_off,
                       int ci_cnt, int Cout, const int* seg_c, int nseg);
int rsu_pack_table_finish(void* host_table, int nentries, int* total_blocks);
/* align (rsu_pack_table_run): dev_table 8. */
int rsu_pack_table_run(const void* dev_table, int nentries, int total_blocks, rsu_stream_t stream);

/* ---- network head / tail (VALU kernels) -------------------------------------------------- */
/* Dropout (unet.py:29-30, 64-65: tf.nn.dropout(net, keep) = net / keep * floor(keep + U[0,1))) is fused into the producer of
 * every tensor it applies to. `keep` in (0, 1]; 1.0 = identity (inference, --dropout=1.0). U is a counter-based hash of
 * (`key`, NHWC element index) -- TensorFlow's Philox stream cannot be reproduced; the parity tests restate the hash bit
 * for bit on the CPU. The host picks one key per dropout site and step. The backward kernels take the same (keep, key). */
/* unet.py:22-23  net = conv1x1(X - 0.5) (color_space_adjust), then the level-0 dropout. x: f32 [npix][3].
 * out16: bf16 [npix][16] = {dropout(net0)[0..2], 0, m[cj]*(x-0.5)[ci] at 4+3*ci+cj, m[0..2] at 13..15} (m = 0/1 keep
 * mask, all ones without dropout) -- channels 0..2 feed the first 3x3 conv, channels 4..15 are kept for the weight and
 * bias gradients of color_space_adjust (rsu_conv_first_bwd_weight). */
/* limit: out16, npix * 32 bytes (the dropout counter 3 * npix + c then stays below 2^28). */
/* align (rsu_color_adjust_fwd): x 4, w 4, b 4, out16 16. */
int rsu_color_adjust_fwd(const float* x, const float* w, const float* b, void* out16, long npix, float keep, unsigned key,
                         rsu_stream_t stream);
/* unet.py:34-35,42-43 first 3x3 conv of level 0 (Cin = 3) + bias + ReLU, dil = 1 or 2 (dilated branch).
 * in16 as above [N][H][W][16]; packed = rsu_pack_conv_first(w f32 HWIO [3][3][3][Cout]) (rows for channels 3..15 are
 * zero, so the (x-0.5) copy in channels 4..6 does not contribute); y bf16 [N][H-2d][W-2d][Cout]. */
/* limit: max(in16 = N*H*W*32, y = N*(H-2d)*(W-2d)*Cout*2) bytes. */
size_t rsu_packed_first_bytes(int Cout);
/* align (rsu_pack_conv_first): w_hwio 4, packed 2. */
int rsu_pack_conv_first(const float* w_hwio, void* packed, int Cout, rsu_stream_t stream);
/* align (rsu_conv_first_fwd): in16 16, packed 16, b 4, y 16. */
int rsu_conv_first_fwd(const void* in16, const void* packed, const float* b, void* y, int N, int H, int W, int Cout,
                       int dil, int ncu, rsu_stream_t stream);
/* unet.py:22-23 AND unet.py:34-35,42-43 in one launch (no dropout: keep == 1): y = relu(conv3x3(conv1x1(x - 0.5, w0) + b0, W1, dilation) + b) straight from
 * the f32 input x [N][H][W][3]; w0 f32 [3][3] ([ci][cj]), b0 f32 [3] (device pointers: color_space_adjust/kernel, /bias); packed, b, y as
 * rsu_conv_first_fwd. The 16-channel tensor of rsu_color_adjust_fwd is neither written nor read (-58 MB and one launch per forward pass at
 * B = 4, 572 px); the results are bit-identical to rsu_color_adjust_fwd(keep = 1) + rsu_conv_first_fwd. A training step still calls
 * rsu_color_adjust_fwd (rsu_conv_first_bwd_weight reads its output), but may do so on another stream, off the forward pass's critical path. */
/* limit: max(x = N*H*W*12, y = N*(H-2d)*(W-2d)*Cout*2) bytes (y always reaches it first: Cout >= 8). */
/* align (rsu_color_conv_first_fwd): x 4, w0 4, b0 4, packed 16, b 4, y 16. */
int rsu_color_conv_first_fwd(const float* x, const float* w0, const float* b0, const void* packed, const float* b, void* y, int N, int H,
                             int W, int Cout, int dil, int ncu, rsu_stream_t stream);
/* weight/bias gradients of that conv and, through it, of color_space_adjust (no input-gradient pass is needed):
 * dw1 [3][3][3][Cout]; gx [9][12][Cout]: rows 0..8 gxc[t][3*ci+cj][co] = sum_pix m[pix+t][cj] (x-0.5)[pix+t][ci] dz[pix][co],
 * rows 9..11 gm[t][cj][co] = sum_pix m[pix+t][cj] dz[pix][co]. With W1 = this conv's kernel:
 *   d(color_space_adjust/kernel)[ci][cj] = 1/keep * sum_{t,co} W1[t][cj][co] gxc[t][3*ci+cj][co]
 *   d(color_space_adjust/bias)[cj]       = 1/keep * sum_{t,co} W1[t][cj][co] gm[t][cj][co]
 * ws: float workspace of rsu_conv_first_bwd_ws_floats() floats. It need not be cleared and holds nothing between calls. */
size_t rsu_conv_first_bwd_ws_floats(int Cout);
/* db (optional): BiasAddGrad of this conv, computed by the same launch. limit: max(in16 = N*H*W*32, dz = N*(H-2d)*(W-2d)*Cout*2) bytes
 * (igemm_wg1's own bound of 2^28 output pixels lies beyond it: 2^28 pixels of in16 are 8 GiB). */
/* align (rsu_conv_first_bwd_weight): in16 16, dz 16, dw1 4, gx 4, db 16, ws 16. */
int rsu_conv_first_bwd_weight(const void* in16, const void* dz, float* dw1, float* gx, float* db, float* ws, int N,
                              int H, int W, int Cout, int dil, int ncu, rsu_stream_t stream);
/* The two sums above in one launch: dW0 f32 [3][3] ([ci][cj]) and db0 f32 [3] from gx [9][12][Cout] and W1 f32 HWIO
 * [3][3][3][Cout]; scale = 1/keep. accumulate != 0 adds to dW0/db0 (the dilated twin conv_dilut_0 shares color_space_adjust). */
/* align (rsu_color_adjust_bwd): gx 4, w1 4, dW0 4, db0 4. */
int rsu_color_adjust_bwd(const float* gx, const float* w1, float* dW0, float* db0, int Cout, float scale, int accumulate,
                         rsu_stream_t stream);
/* unet.py:95 weight_output 1x1 conv (C -> 2) fused with tf_aerial_images.py:147-148 softmax[...,1].
 * act bf16 [npix][C]; w f32 [C][2]; prob f32 [npix]; logits f32 [npix][2] or NULL (unet.forward's return value). */
/* limit (this and every rsu_head_* entry below, rsu_loss.h and rsu_cldice.h included): act (and dact), npix * C * 2 bytes -- with C >= 8
 * the largest tensor of the call (labels and logits are 8 bytes per pixel). */
/* align (rsu_head_fwd): act 16, w 4, b 4, prob 4, logits 4. */
int rsu_head_fwd(const void* act, const float* w, const float* b, float* prob, float* logits, long npix, int C,
                 rsu_stream_t stream);
/* Same plus tf_aerial_images.py:103-110 mean sparse softmax cross-entropy and its backward:
 * labels int64 [npix] in {0,1}; loss_sum f32[1] (+= sum of per-pixel losses; caller zeroes it);
 * dact bf16 [npix][C] = gradient wrt the PRE-activation of the last conv2 (ReLU mask applied),
 * scaled by inv_count (1 / global pixel count); dw f32 [C][2], db f32 [2] (overwritten).
 * ws: rsu_head_ws_floats(npix, C) floats. It need not be cleared and holds nothing between calls. */
size_t rsu_head_ws_floats(long npix, int C);
/* align (rsu_head_fwd_bwd): act 16, w 4, b 4, labels 8, prob 4, loss_sum 4, dact 16, dw 4, db 4, ws 4. */
int rsu_head_fwd_bwd(const void* act, const float* w, const float* b, const int64_t* labels, float* prob,
                     float* loss_sum, void* dact, float* dw, float* db, float* ws, long npix, int C,
                     float inv_count, rsu_stream_t stream);
/* The weighted form of tf_aerial_images.py:103-110: tf.losses.sparse_softmax_cross_entropy(labels, logits, weights) with
 * reduction SUM_OVER_BATCH_SIZE, the U-Net paper's weight-map loss. Per pixel p with label l_p and CE_p = -log softmax(z_p)[l_p]:
 *   omega_p = 0 if l_p is neither 0 nor 1 (an IGNORED pixel; the test is made on all 64 bits of the label),
 *           = class_w[l_p] * pixel_w[p] otherwise   (class_w: device f32[2] or NULL = {1, 1}; pixel_w: device f32[npix] or NULL = 1)
 *   loss_sum += sum_p omega_p CE_p;  weight_sum (f32[1] or NULL) += sum_p omega_p;  dlogits_p = omega_p (softmax(z_p) - onehot(l_p)) inv_count
 * inv_count stays 1 / (global pixel count): NOT 1 / sum omega (no second pass, no device-side scalar in front of the gradient, and the
 * SUM all-reduce of per-rank gradients stays correct); weight_sum lets a host REPORT loss_sum / weight_sum. The caller zeroes loss_sum
 * and weight_sum. prob is written for every pixel; an ignored pixel's dact row is +0 and it adds nothing to dw, db, loss_sum,
 * weight_sum, whatever its pixel_w holds (it is never multiplied). dact, dw, db, prob, inv_count, C and the error codes are
 * rsu_head_fwd_bwd's. Same grid, pixel-to-thread mapping and fixed summation orders: results are deterministic, and with every
 * omega_p == 1 (class_w {1, 1} or NULL, pixel_w all ones or NULL, labels in {0,1}) they equal rsu_head_fwd_bwd's bit for bit.
 * ws: rsu_head_w_ws_floats(npix, C) floats (one more partial per workgroup than rsu_head_ws_floats). It need not be cleared and holds nothing between calls. */
size_t rsu_head_w_ws_floats(long npix, int C);
/* align (rsu_head_fwd_bwd_w): act 16, w 4, b 4, labels 8, class_w 4, pixel_w 4, prob 4, loss_sum 4, weight_sum 4, dact 16, dw 4, db 4, ws 4. */
int rsu_head_fwd_bwd_w(const void* act, const float* w, const float* b, const int64_t* labels, const float* class_w,
                       const float* pixel_w, float* prob, float* loss_sum, float* weight_sum, void* dact, float* dw, float* db,
                       float* ws, long npix, int C, float inv_count, rsu_stream_t stream);
/* The soft-Dice (soft-F1) term next to that cross-entropy: loss = sum_p omega_p CE_p inv_count + dice_scale (1 - D). With
 * p_i = softmax(z_i)[1] (the value written to prob), y_i = 1 for label 1 and 0 otherwise, and the Dice mass of a pixel
 *   m_i = 0 if its label is neither 0 nor 1 (all 64 bits tested; by selection, never by multiplication),
 *       = pixel_w[i] otherwise (1 where pixel_w is NULL); class_w does NOT enter the Dice term, it stays the cross-entropy's:
 *   I = sum m_i p_i y_i    P = sum m_i p_i    Y = sum m_i y_i    (over the npix pixels of the call: the rank's batch)
 *   U = P + Y + smooth     D = (2 I + smooth) / U                 (smooth > 0)
 *   d(1 - D)/dz_i[1] = m_i (D - 2 y_i) / U p_i (1 - p_i) = -d(1 - D)/dz_i[0]
 * Every pixel's gradient needs the three batch-wide sums, so the head runs twice, and a device-resident scalar buffer sits between the
 * two launches (the one exception to "no device-side scalar in front of the gradient" above; only a step that asks for Dice pays it):
 *   rsu_head_dice_sums     forward only: writes prob and OVERWRITES dice_sums[0..2] = {I, P, Y} (f32[3]; nothing to zero), fixed orders.
 *   rsu_head_fwd_bwd_dice  rsu_head_fwd_bwd_w plus dice_scale * d(1 - D)/dz on the logits' gradients in front of dact, dw and db; it READS
 *                          {I, P, Y} from dice_sums and recomputes none of them. loss_sum and weight_sum keep rsu_head_fwd_bwd_w's
 *                          meaning (cross-entropy only, caller zeroes them); a host adds dice_scale (1 - D) from dice_sums for reporting.
 * The two calls on one stream need no host synchronisation and no device-to-host copy between them. dice_sums is an ordinary device
 * buffer that the caller owns between the calls: a host may combine it across ranks there (nothing here does: each rank's term is its
 * own batch's Dice, and dice_scale = lambda / world keeps the SUM all-reduce of gradients the gradient of the mean of the ranks' terms).
 * An ignored pixel's dact row is +0 and it adds nothing to any sum, whatever its pixel_w holds. Errors: rsu_head_fwd_bwd_w's, plus
 * RSU_EINVAL for dice_sums == NULL, a smooth that is not finite and > 0, a dice_scale that is not finite and >= 0 -- returned before
 * anything is launched or written. ws: rsu_head_dice_ws_floats(npix, C) floats, enough for either call.
 * It need not be cleared and holds nothing between calls, not between these two either: rsu_head_dice_sums writes dice_sums = {I, P, Y},
 * rsu_head_fwd_bwd_dice reads them from there; each call's partial sums live in ws from its first launch to its second. */
size_t rsu_head_dice_ws_floats(long npix, int C);
/* align (rsu_head_dice_sums): act 16, w 4, b 4, labels 8, pixel_w 4, prob 4, dice_sums 4, ws 4. */
int rsu_head_dice_sums(const void* act, const float* w, const float* b, const int64_t* labels, const float* pixel_w, float* prob,
                       float* dice_sums, float* ws, long npix, int C, rsu_stream_t stream);
/* align (rsu_head_fwd_bwd_dice): act 16, w 4, b 4, labels 8, class_w 4, pixel_w 4, dice_sums 4, prob 4, loss_sum 4, weight_sum 4, dact 16, dw 4,
 * db 4, ws 4. */
int rsu_head_fwd_bwd_dice(const void* act, const float* w, const float* b, const int64_t* labels, const float* class_w,
                          const float* pixel_w, const float* dice_sums, float dice_scale, float smooth, float* prob, float* loss_sum,
                          float* weight_sum, void* dact, float* dw, float* db, float* ws, long npix, int C, float inv_count,
                          rsu_stream_t stream);
/* The evaluation head, for held-out data: forward only (no dact, dw, db), one call per batch, every output an ACCUMULATOR that the
 * caller zeroes once in front of a whole validation set and reads back once behind it. Logits, softmax and prob are the other heads'
 * (same bits). With omega_p of rsu_head_fwd_bwd_w and {I, P, Y}, m_i of rsu_head_dice_sums over the npix pixels of the call:
 *   sums[0..4] (f32[5]) += {sum omega CE, sum omega, I, P, Y}
 *   hist[l][min(RSU_EVAL_BINS - 1, (int)(p * RSU_EVAL_BINS))] += 1   for every pixel with label l in {0, 1} (whatever its weights are),
 *                                                                   p the f32 value written to prob; hist is u64 [2][RSU_EVAL_BINS]
 * A label that is neither 0 nor 1 (all 64 bits tested) ignores its pixel by selection: prob is written, nothing else sees it, whatever
 * its pixel_w holds. class_w (f32[2]) and pixel_w (f32[npix]) may be NULL (= 1). Same grid, pixel-to-thread mapping and fixed summation
 * orders as the training heads: from zeroed accumulators sums[0..1] equal rsu_head_fwd_bwd_w's loss_sum / weight_sum and sums[2..4]
 * equal rsu_head_dice_sums's dice_sums bit for bit; the histogram holds integer counts (vector 64-bit atomics of per-launch totals),
 * so every output is deterministic. With a threshold t = k / RSU_EVAL_BINS, "p >= t" is "bin >= k" exactly: the confusion counts at
 * every such threshold follow from hist on the host. Errors: RSU_EINVAL for a NULL act, w, b, labels, prob, sums, hist or ws, a C
 * the other heads refuse, npix < 1 -- returned before anything is launched or written.
 * ws: rsu_head_eval_ws_floats(npix, C) floats (0 for a refused C or npix). It need not be cleared and holds nothing between calls. */
#define RSU_EVAL_BINS 256
size_t rsu_head_eval_ws_floats(long npix, int C);
/* align (rsu_head_eval): act 16, w 4, b 4, labels 8, class_w 4, pixel_w 4, prob 4, sums 4, hist 8, ws 4. */
int rsu_head_eval(const void* act, const float* w, const float* b, const int64_t* labels, const float* class_w, const float* pixel_w,
                  float* prob, float* sums, unsigned long long* hist, float* ws, long npix, int C, rsu_stream_t stream);

/* The border-distance weight map (new): the producer of pixel_w above, the U-Net paper's w0 exp(-(d1 + d2)^2 / (2 sigma^2)) restated for a
 * two-class semantic mask (no instances: the distance is to the other class; the paper's class-balancing term w_c stays class_w).
 * For a batch of label tiles labels int64 [N][H][W], per tile n, PATCH-LOCAL (only pixels of the same tile are looked at: a training patch
 * does not see the ground truth outside its window, so a border just beyond the patch edge is not felt):
 *   a label is VALID if it is 0 or 1 (all 64 bits tested, as in the heads);
 *   D2(p) = min (dy^2 + dx^2) over the valid pixels q of the tile with label 1 - l_p, for a valid p: the exact integer squared Euclidean
 *           distance to the other class (border pixels have D2 = 1); RSU_BORDER_D2_INF where the tile holds no valid pixel of that class;
 *   border(p) = 1 + w0 exp(-D2(p) / (2 sigma^2)) in float32, exactly 1 where D2 is infinite;
 *   out[p] = (mul ? mul[p] : 1) * border(p)       mul: an optional caller map f32 [N][H][W] (how a caller's own weight map combines);
 *   an IGNORED pixel (any other label): out = +0, d2 = RSU_BORDER_D2_INF; it is never anyone's "other class" and its mul is never read
 *   (selection, not multiplication, as everywhere in the head family).
 * out f32 [N][H][W]; d2 int32 [N][H][W] or NULL; ws: rsu_border_map_ws_bytes(N, H, W) bytes (0 for a refused size).
 * It need not be cleared and holds nothing between calls (the column pass writes every word the row pass reads).
 * Exact separable transform in integer arithmetic (a column pass into ws, a row pass from LDS): d2 is exact and no output depends on the
 * grid, the wave order or the box; exp is a fixed sequence of float32 operations (no library call), which hostio.border_weight_map
 * restates: out is reproducible bit for bit on the host. Two launches on `stream`, no host synchronisation, no allocation, no atomics.
 * Supported: 1 <= H, W <= RSU_BORDER_MAX_SIDE (every patch_size of the training hosts; 388 included), N >= 1. Errors, returned before
 * anything is launched or written: RSU_EINVAL for a NULL labels, out or ws, N, H or W below 1, H or W above RSU_BORDER_MAX_SIDE (the
 * row staging; there is no slower path), a w0 that is not finite and >= 0, a sigma that is not finite and > 0; RSU_E2BIG when the label
 * tensor reaches 2 GiB. */
#define RSU_BORDER_D2_INF 0x7fffffff
#define RSU_BORDER_MAX_SIDE 1024
size_t rsu_border_map_ws_bytes(int N, int H, int W);
/* align (rsu_border_map): labels 8, mul 4, out 4, d2 4, ws 4. */
int rsu_border_map(const int64_t* labels, const float* mul, float* out, int32_t* d2 /* may be NULL */, void* ws,
                   int N, int H, int W, float w0, float sigma, rsu_stream_t stream);

/* ---- 3x3 convolution, MFMA implicit GEMM -------------------------------------------------- */
/* unet.py:34-39,42-45,88-91: y = relu(conv3x3_valid(concat(srcs), W, dilation) + b).
 * All sources share the window size (Hin, Win); y is bf16 [N][Hin-2d][Win-2d][Cout]. */
/* limit (rsu_conv2d_fwd, _fwd_pool, _bwd_data and their _k forms): the output, and EVERY source as a whole, N * H * W * C * 2 bytes of the
 * uncropped tensor (a cropped skip tensor is larger than its window). */
/* align (rsu_conv2d_fwd): srcs host, srcs.ptr 16, packed_fwd 16, bias 4, y 16. */
int rsu_conv2d_fwd(const rsu_src_t* srcs, int nsrc, const void* packed_fwd, const float* bias, void* y, int N,
                   int Hin, int Win, int Cout, int dil, int relu, int ncu, rsu_stream_t stream);
/* The same three launches (rsu_conv2d_fwd, rsu_conv2d_fwd_pool, rsu_conv2d_bwd_data) with a caller-owned workspace `kws` of `kws_floats`
 * floats (rsu_conv_splitk_ws_floats() is always enough; NULL / 0 = the plain entry points). A layer with far fewer (pixel tile, channel
 * block) pairs than CUs -- the deep levels of the U-Net at small batches: 18x18 .. 66x66 pixels, 512 .. 2048 channels -- may then cut its
 * reduction (taps x input channels) into up to 16 slices, one workgroup per (tile, block, slice): the slices' fp32 partial sums go to
 * `kws` and a second launch sums them IN SLICE ORDER (deterministic), adds nothing else (the bias rides in slice 0), applies ReLU /
 * the ReLU mask and stores bf16. Results equal the unsplit launch up to the association of the fp32 sum over the slices. Whether a launch
 * splits, and into how many slices, is a pure function of its geometry (N, output size, channel counts, dilation) -- never of the CU
 * budget, the tuning table or a measurement: the same launch sums in the same order in every schedule and on every box (RSU_KSPLIT=0:
 * never split). The geometry includes the batch: a layer splits into more slices at N = 1 than at N = 4, so the deep layers of one image
 * associate their fp32 sums differently in batches of different size (the distance is pinned per layer in tests/test_gpu_ops.py; making
 * the rule batch-independent cost the N = 4 step 12-14 %, profiles/r05/abenv_perimg_*.txt). The workspace must not be shared with a launch
 * running concurrently on another stream: the host keeps one per stream that issues conv launches. kws need not be cleared and holds
 * nothing between calls: the first launch writes every partial sum the second reads, and one buffer serves every layer in turn. */
size_t rsu_conv_splitk_ws_floats(void);
/* align (rsu_conv2d_fwd_k): srcs host, srcs.ptr 16, packed_fwd 16, bias 4, y 16, kws 16. */
int rsu_conv2d_fwd_k(const rsu_src_t* srcs, int nsrc, const void* packed_fwd, const float* bias, void* y, int N,
                     int Hin, int Win, int Cout, int dil, int relu, int ncu, float* kws, size_t kws_floats, rsu_stream_t stream);
/* align (rsu_conv2d_fwd_pool_k): srcs host, srcs.ptr 16, packed_fwd 16, bias 4, y 16, pooled 16, code 8, kws 16. */
int rsu_conv2d_fwd_pool_k(const rsu_src_t* srcs, int nsrc, const void* packed_fwd, const float* bias, void* y, void* pooled, void* code,
                          int N, int Hin, int Win, int Cout, float keep, unsigned key, int ncu, float* kws, size_t kws_floats, rsu_stream_t stream);
/* align (rsu_conv2d_bwd_data_k): dz 16, packed_bwd 16, dx 16, relu_src 16, kws 16. */
int rsu_conv2d_bwd_data_k(const void* dz, const void* packed_bwd, void* dx, const void* relu_src, int accumulate, int N, int H, int W,
                          int Cin_total, int ci_off, int ci_cnt, int Cout, int dil, int ncu, float* kws, size_t kws_floats, rsu_stream_t stream);
/* unet.py:44-52 in one launch: y = relu(conv3x3_valid(concat(srcs), W) + b) (dilation 1), pooled = max_pooling2d(y, 2, 2) followed by
 * the next level's dropout (keep, key as rsu_maxpool2x2_fwd), and -- code != NULL -- the code bytes of rsu_maxpool2x2_fwd_code.
 * With code != NULL the conv's output size must be even (RSU_EINVAL before anything is launched otherwise); without code bytes odd
 * sizes pool with floor semantics, as max_pooling2d does. Where a tile shape with whole 2x2 windows per wavefront fits the layer, the
 * size is even and keep == 1 the pool is part of the conv kernel's epilogue (lane shuffles on the packed results; the activation is not
 * read back from HBM); otherwise the call issues the two launches itself. Same bits either way. */
/* align (rsu_conv2d_fwd_pool): srcs host, srcs.ptr 16, packed_fwd 16, bias 4, y 16, pooled 16, code 8. */
int rsu_conv2d_fwd_pool(const rsu_src_t* srcs, int nsrc, const void* packed_fwd, const float* bias, void* y, void* pooled, void* code,
                        int N, int Hin, int Win, int Cout, float keep, unsigned key, int ncu, rsu_stream_t stream);
/* Conv2DBackpropInput for input channels [ci_off, ci_off+ci_cnt) of a conv with Cin_total inputs:
 * dx bf16 [N][H][W][ci_cnt] (H, W = conv input size), dz bf16 [N][H-2d][W-2d][Cout].
 * relu_src (optional, same shape as dx): dx *= (relu_src > 0)  -- ReluGrad of the producing layer.
 * accumulate != 0: dx += result (two consumers of one tensor, unet.py:32-45). */
/* align (rsu_conv2d_bwd_data): dz 16, packed_bwd 16, dx 16, relu_src 16. */
int rsu_conv2d_bwd_data(const void* dz, const void* packed_bwd, void* dx, const void* relu_src, int accumulate,
                        int N, int H, int W, int Cin_total, int ci_off, int ci_cnt, int Cout, int dil, int ncu,
                        rsu_stream_t stream);
/* Conv2DBackpropFilter for the input channels held by `src` (rows [ci_off, ci_off+src.C) of dw):
 * dw f32 HWIO [3][3][Cin_total][Cout] (only those rows are written). (Ho, Wo) = size of dz.
 * ws: rsu_conv2d_bwd_weight_ws_floats() floats of scratch (split-K slabs). It need not be cleared and holds nothing between calls. */
size_t rsu_conv2d_bwd_weight_ws_floats(int Cin_total, int src_C, int Cout);
/* db (optional, f32 [Cout]): BiasAddGrad = sum over pixels of dz, computed by the same launch (one extra MFMA per
 * 32-pixel step); pass it with ONE of the sources of a concatenated input, NULL with the others.
 * limit: max(src as a whole = N*src.H*src.W*src.C*2, dz = N*Ho*Wo*Cout*2) bytes ("beyond that the offsets wrapped"); rsu_wgrad_group_plan
 * returns the same RSU_E2BIG for any of its jobs. */
/* align (rsu_conv2d_bwd_weight): src host, src.ptr 16, dz 16, dw 16, db 16, ws 16. */
int rsu_conv2d_bwd_weight(const rsu_src_t* src, const void* dz, float* dw, float* db, float* ws, int N, int Ho, int Wo,
                          int Cin_total, int ci_off, int Cout, int dil, int ncu, rsu_stream_t stream);
/* Grouped weight gradients (new; TensorFlow's executor runs independent Conv2DBackpropFilter ops side by side, tf_aerial_images.py:120-121).
 * A weight-gradient launch that has the chip to itself writes one fp32 partial result per workgroup -- 75 MB of slabs per layer on
 * 256 CUs, read back by a reduce launch -- and a layer with few pixels cannot fill the chip. A GROUP runs up to
 * RSU_WGRAD_GROUP_MAX layers in ONE launch: every layer gets a share of the chip in proportion to its work, the shallow layers are
 * split over few workgroups (the slabs of the whole group are about one per CU), the deep ones not at all (their workgroups write the
 * gradient in place), and ONE reduce launch finishes all splits. Results equal those of the single launches up to the summation
 * order of the pixel splits (fp32 rounding), and are deterministic for a given (jobs, N, ncu).
 * Usage (the pattern of rsu_pack_table_*): fill a host table with rsu_wgrad_group_plan (the pointers are static for a network, so this
 * happens once per group and CU budget), copy its rsu_wgrad_group_table_bytes() bytes to the device once, then call
 * rsu_wgrad_group_run after every backward pass. job.kind selects the fields' meaning:
 *   RSU_WGRAD_CONV3X3  as rsu_conv2d_bwd_weight: src = the input window, dz [N][Ho][Wo][Cout], dw HWIO rows [ci_off, ci_off+src.C), db optional
 *   RSU_WGRAD_CONVT2X2 as rsu_convT2x2_bwd_weight: src = {x, H, W, Cin, 0, 0}, dz = dy [N][2H][2W][Cout], dw = dK, db optional
 * ws: rsu_wgrad_group_ws_floats() floats of scratch, owned by the group between a run and the end of its stream work. rsu_wgrad_group_plan
 * only stores the address; every run writes the slabs its reduce launch reads. It need not be cleared and holds nothing between runs:
 * other launches may use it in between. */
#define RSU_WGRAD_CONV3X3 0
#define RSU_WGRAD_CONVT2X2 1
#define RSU_WGRAD_GROUP_MAX 16
typedef struct {
    int kind;
    rsu_src_t src;
    const void* dz;
    float* dw;
    float* db;
    int Ho, Wo;                         /* RSU_WGRAD_CONV3X3: size of dz */
    int Cin_total, ci_off, Cout, dil;   /* RSU_WGRAD_CONVT2X2 reads Cout only */
} rsu_wgrad_job_t;
size_t rsu_wgrad_group_table_bytes(void);
size_t rsu_wgrad_group_ws_floats(void);
/* align (rsu_wgrad_group_plan): jobs host, jobs.db 16, jobs.dw 16, jobs.dz 16, jobs.src.ptr 16, ws 16, host_table host. */
int rsu_wgrad_group_plan(const rsu_wgrad_job_t* jobs, int njobs, float* ws, int N, int ncu, void* host_table);
/* align (rsu_wgrad_group_run): host_table host, dev_table 8. */
int rsu_wgrad_group_run(const void* host_table, const void* dev_table, rsu_stream_t stream);
/* BiasAddGrad: db[c] = sum over npix of dz[pix][c]. ws: rsu_bias_grad_ws_floats(npix, C) floats. It need not be cleared and holds nothing between calls. */
/* limit: dz, npix * C * 2 bytes. */
size_t rsu_bias_grad_ws_floats(long npix, int C);
/* align (rsu_bias_grad): dz 16, db 4, ws 4. */
int rsu_bias_grad(const void* dz, float* db, float* ws, long npix, int C, rsu_stream_t stream);

/* ---- 2x2 max pool -------------------------------------------------------------------------- */
/* unet.py:52 max_pooling2d (2,2)/(2,2) VALID, then the next level's dropout (unet.py:29-30; keep = 1: none).
 * x bf16 [N][H][W][C] -> y [N][H/2][W/2][C] */
/* limit (both forms): x, N*H*W*C*2 bytes (the dropout counter, a pooled element index, then stays below 2^28). */
/* align (rsu_maxpool2x2_fwd): x 16, y 16. */
int rsu_maxpool2x2_fwd(const void* x, void* y, int N, int H, int W, int C, float keep, unsigned key,
                       rsu_stream_t stream);
/* ... and, for training, a code tensor for the gradient junction below (H, W even; code [N][H/2][W/2][C] bytes, may be NULL):
 * per pooled element bits 0-3 = (window element 2*dy+dx > 0), bits 4-5 = the window's first maximum in row-major order. */
/* align (rsu_maxpool2x2_fwd_code): x 16, y 16, code 8. */
int rsu_maxpool2x2_fwd_code(const void* x, void* y, void* code, int N, int H, int W, int C, float keep, unsigned key,
                            rsu_stream_t stream);
/* Gradient junction at an encoder output y_act (ReLU output, bf16 [N][H][W][C]):
 *   g = MaxPoolGrad(y_act, dropout_grad(dpool))  (dpool bf16 [N][H/2][W/2][C], may be NULL; (keep, key) as in
 *                                             rsu_maxpool2x2_fwd: dpool is the gradient of the DROPPED pooled tensor)
 *     + zero-pad(dskip)                      (dskip bf16 [N][Hs][Ws][C] centred, may be NULL;
 *                                             adjoint of the centre crop of unet.py:70-83)
 *   dz = g * (y_act > 0)                     (ReluGrad) -> bf16 [N][H][W][C]
 * MaxPoolGrad routes to the first maximum of the window in row-major order.
 * limit (both forms): dz (= y_act), N*H*W*C*2 bytes: the int row count N * (H / 2) and pooled element index of the code-byte kernel and the
 * 32-bit dropout counter of both kernels then stay below 2^28. */
/* align (rsu_pool_skip_relu_bwd): y_act 16, dpool 16, dskip 16, dz 16. */
int rsu_pool_skip_relu_bwd(const void* y_act, const void* dpool, const void* dskip, void* dz, int N, int H, int W,
                           int C, int Hs, int Ws, float keep, unsigned key, rsu_stream_t stream);
/* The same junction from the code tensor of rsu_maxpool2x2_fwd_code instead of the activation (y_act may then be NULL): one
 * byte per pooled element instead of four bf16 activations, the same bits. */
/* align (rsu_pool_skip_relu_bwd_code): y_act 16, code 8, dpool 16, dskip 16, dz 16. */
int rsu_pool_skip_relu_bwd_code(const void* y_act, const void* code, const void* dpool, const void* dskip, void* dz, int N,
                                int H, int W, int C, int Hs, int Ws, float keep, unsigned key, rsu_stream_t stream);
/* unet.py:64-65 dropout in front of a transposed conv: y = x / keep * floor(keep + U), bf16 [n] -> bf16 [n] (n % 8 == 0).
 * Its backward is fused into rsu_convT2x2_bwd_data: pass y as relu_src (y > 0 <=> x > 0 and kept) and out_scale = 1/keep. */
/* limit: n * 2 bytes (the dropout counter is the element index, then below 2^30); an n that is no multiple of 8 is RSU_EINVAL first. */
/* align (rsu_dropout_fwd): x 16, y 16. */
int rsu_dropout_fwd(const void* x, void* y, long n, float keep, unsigned key, rsu_stream_t stream);

/* ---- 2x2 stride-2 transposed convolution (unet.py:67-68) ---------------------------------- */
/* limit (all three): max(x = N*H*W*Cin*2, y / dy = N*4*H*W*Cout*2) bytes. The faster kernels' own bounds (igemm_ct: the 4x tensor below the
 * limit; igemm_wgt: 2^28 input pixels) select no slower path that could run: the generic launches behind them refuse the same tensors,
 * and 2^28 pixels of 8 channels are 4 GiB. */
/* align (rsu_convT2x2_fwd): x 16, packed_fwd 16, bias 4, y 16. */
int rsu_convT2x2_fwd(const void* x, const void* packed_fwd, const float* bias, void* y, int N, int H, int W,
                     int Cin, int Cout, int ncu, rsu_stream_t stream);
/* dx bf16 [N][H][W][Cin] = out_scale * sum_{a,b,co} dy[2i+a][2j+b][co] K[a][b][co][ci], times (relu_src > 0) if given.
 * out_scale != 1 is applied by a second pass over the stored tensor: dx = bf16(out_scale * bf16(sum)), two roundings by design
 * (tests/test_gpu_rounding.py holds it to exactly these two). */
/* align (rsu_convT2x2_bwd_data): dy 16, packed_bwd 16, dx 16, relu_src 16. */
int rsu_convT2x2_bwd_data(const void* dy, const void* packed_bwd, void* dx, const void* relu_src, float out_scale,
                          int N, int H, int W, int Cin, int Cout, int ncu, rsu_stream_t stream);
/* dK f32 [2][2][Cout][Cin] and, when db != NULL, db f32 [Cout] = sum over all pixels of dy (BiasAddGrad of the transposed
 * conv, unet.py:72) from the same launch; ws: rsu_convT2x2_bwd_weight_ws_floats() floats. It need not be cleared and holds nothing between calls. */
size_t rsu_convT2x2_bwd_weight_ws_floats(int Cin, int Cout);
/* align (rsu_convT2x2_bwd_weight): x 16, dy 16, dK 16, db 16, ws 16. */
int rsu_convT2x2_bwd_weight(const void* x, const void* dy, float* dK, float* db, float* ws, int N, int H, int W,
                            int Cin, int Cout, int ncu, rsu_stream_t stream);

/* ---- optimizer (tf_aerial_images.py:116-121, MomentumOptimizer, use_nesterov=False) ------- */
/* acc = mu*acc + gscale*g ; w -= lr*acc. gscale folds the 1/world_size of data-parallel averaging. */
/* align (rsu_momentum_step): w 16, acc 16, g 16. */
int rsu_momentum_step(float* w, float* acc, const float* g, float lr, float mu, float gscale, long n,
                      rsu_stream_t stream);

/* The Momentum step of EVERY live variable and the re-pack of the MFMA copies in ONE launch (new): rsu_momentum_step moves 20 B per
 * parameter and the batched re-pack reads every conv kernel twice more; this pass reads w, acc, g once, writes w, acc and both packed
 * layouts: 24 B per weight. Same arithmetic per element as rsu_momentum_step, same packed bits as rsu_pack_*. Usage (the pattern of
 * rsu_pack_table_*): one table entry per variable -- rsu_update_table_add for a conv / transposed-conv kernel with its packed buffers
 * (kind RSU_PACK_CONV_FWD: packed_fwd + one backward-data pack per concat source in packed_bwd[0..nseg), or packed_bwd = NULL for a
 * forward-only net; RSU_PACK_CONVT_FWD: packed_fwd (four matrices) + packed_bwd[0]; RSU_PACK_CONV_FIRST: packed_fwd only),
 * rsu_update_table_add_plain for everything no MFMA kernel reads (biases, colour adjust, the 1x1 head; w / acc / g 16-byte aligned) --
 * then rsu_update_table_finish, copy the table to the device once, and rsu_update_table_run after every backward pass. The pass
 * rewrites the 32 x 32 blocks of a packed buffer that hold weights; the zero padding beyond them (rows up to a multiple of 128) is not
 * written again (rewriting it every step would cost the pass bandwidth for bytes that never change): every packed buffer of a table must
 * have been packed ONCE by rsu_pack_* / rsu_pack_table_run (from the initial weights) before the first run. */
size_t rsu_update_table_entry_bytes(void);
/* align (rsu_update_table_add_plain): host_table host, w 16, acc 16, g 16. */
int rsu_update_table_add_plain(void* host_table, int index, float* w, float* acc, const float* g, long n);
/* align (rsu_update_table_add): host_table host, w 16, acc 16, g 16, packed_fwd 16, packed_bwd host, packed_bwd[] 16, seg_c host. */
int rsu_update_table_add(void* host_table, int index, int kind, float* w, float* acc, const float* g, void* packed_fwd,
                         void* const* packed_bwd, int Cin_total, int Cout, const int* seg_c, int nseg);
int rsu_update_table_finish(void* host_table, int nentries, int* total_blocks);
/* align (rsu_update_table_run): dev_table 8. */
int rsu_update_table_run(const void* dev_table, int nentries, int total_blocks, float lr, float mu, float gscale,
                         rsu_stream_t stream);

/* ---- optimizer: tf.train.AdamOptimizer (new; the reference trains with Momentum only) -------- */
/* TensorFlow 1.x ApplyAdam, float32, in this order (IEEE sqrt and divide, no contraction):
 *   g' = gscale*g ; m += (g' - m)*(1 - beta1) ; v += (g'*g' - v)*(1 - beta2) ; w -= (m*alpha) / (sqrt(v) + epsilon)
 * with alpha = lr_t * sqrt(1 - beta2^t) / (1 - beta1^t) computed by the caller in float32 (AdamOptimizer._apply_dense; beta1^t and
 * beta2^t are the float32 `beta1_power` / `beta2_power` accumulators, multiplied by beta1 / beta2 after every step as
 * AdamOptimizer._finish does). gscale folds the 1/world_size of data-parallel averaging. w, m, v, g 16-byte aligned. */
/* align (rsu_adam_step): w 16, m 16, v 16, g 16. */
int rsu_adam_step(float* w, float* m, float* v, const float* g, float alpha, float beta1, float beta2, float epsilon, float gscale,
                  long n, rsu_stream_t stream);
/* The Adam step of every live variable and the re-pack of the MFMA copies in ONE launch: the table of rsu_update_table_add[_plain]
 * (its `acc` is Adam's first slot m) plus, per entry, the second slot v given by rsu_update_table_set_second_slot (16-byte aligned,
 * same extent as acc) before rsu_update_table_finish. Reads w, m, v, g once, writes w, m, v and the packed layouts: 32 B per weight of
 * a packed conv kernel, 28 B per plain-range float (Momentum: 24 B and 20 B). Same arithmetic per element as rsu_adam_step, same
 * packed bits as rsu_pack_*. */
/* align (rsu_update_table_set_second_slot): host_table host, v 16. */
int rsu_update_table_set_second_slot(void* host_table, int index, float* v);
/* align (rsu_update_table_run_adam): dev_table 8. */
int rsu_update_table_run_adam(const void* dev_table, int nentries, int total_blocks, float alpha, float beta1, float beta2,
                              float epsilon, float gscale, rsu_stream_t stream);

/* ---- optimizer: clipping by the global norm, with a guard against a gradient that is not finite (new) -------- */
/* rsu_grad_norm leaves the squared norm of g[0, n), the clipping factor for max_norm and three counters in a 32-byte STATE RECORD in
 * device memory; the two _clip update passes below read their scale from that record, so a clipped step needs no host synchronisation.
 * The record (rsu_clip_state_bytes() == RSU_CLIP_STATE_BYTES; 4-byte aligned; the caller zeroes it ONCE, before the first call):
 *   float    sumsq           sum of g[i]^2 (below)
 *   float    norm            (float)sqrt((double)sumsq)
 *   float    scale           norm > max_norm ? (float)((double)max_norm / (double)norm) : 1.0f; 0.0f when bit 1 of flags is set
 *   uint32_t flags           bit 0 RSU_CLIP_CLIPPED: norm > max_norm, scale < 1; bit 1 RSU_CLIP_NONFINITE: an element of g is inf or nan, or
 *                            sumsq is not finite -- an OVERFLOW of the sum of squares included (finite elements near 1e19 and above):
 *                            such a step cannot be scaled and is skipped like one with a nan. The two bits exclude each other
 *   uint32_t steps           calls so far
 *   uint32_t clipped_steps   calls that set bit 0
 *   uint32_t skipped_steps   calls that set bit 1
 *   uint32_t pad             0
 * sumsq, norm, scale and flags describe the last call, the three counters accumulate over the calls.
 * The sum: two launches on `stream`. Pass 1 cuts g into shares of RSU_GRAD_NORM_BLOCK_FLOATS floats, one per 256-lane workgroup -- a grid
 * that depends on n ALONE, not on the CU budget, the device or the autotuner; a lane sums the squares of its 16 float4 in float32 in a
 * fixed order, a fixed tree adds the lanes, and the workgroup writes one partial sum and one "saw inf or nan" word. Pass 2, one
 * workgroup, adds the partials in double in a fixed order and one thread writes the record. The same g, n and max_norm therefore
 * give the same bits on every call, device and rank. Only g[0, n) is read (the n & 3 scalars behind the last float4 singly).
 * ws: rsu_grad_norm_ws_floats(n) floats (2 per workgroup; 0 for n < 1), written in full, nothing behind them. It need not be
 * cleared and holds nothing between calls: what the calls share is `state`.
 * Errors, returned before anything is launched: RSU_EINVAL for a NULL g, ws or state, n < 1, a max_norm that is not > 0 (nan included;
 * +inf is allowed: the call then only measures and guards), a g that is not 16-byte aligned, a ws or state that is not 4-byte aligned. */
#define RSU_CLIP_STATE_BYTES 32
#define RSU_CLIP_CLIPPED 1u
#define RSU_CLIP_NONFINITE 2u
#define RSU_GRAD_NORM_BLOCK_FLOATS 16384
size_t rsu_clip_state_bytes(void);
size_t rsu_grad_norm_ws_floats(long n);
/* align (rsu_grad_norm): g 16, ws 4, state 4. */
int rsu_grad_norm(const float* g, long n, float max_norm, float* ws, void* state, rsu_stream_t stream);
/* rsu_update_table_run / rsu_update_table_run_adam with gscale * state->scale for gscale (one float32 multiply, made once per
 * workgroup; everything behind it is the arithmetic of the plain pass, so a _clip run whose record holds scale s gives the bits of the
 * plain run with gscale * s). `state` is a record rsu_grad_norm wrote earlier on the same stream. With RSU_CLIP_NONFINITE set in it
 * every workgroup returns before its first load: weights, optimizer slots and packed copies stay as they are, consistent with each
 * other. RSU_EINVAL for a NULL or misaligned state (and what the plain run rejects), before anything is launched. */
/* align (rsu_update_table_run_clip): dev_table 8, state 4. */
int rsu_update_table_run_clip(const void* dev_table, int nentries, int total_blocks, float lr, float mu, float gscale,
                              const void* state, rsu_stream_t stream);
/* align (rsu_update_table_run_adam_clip): dev_table 8, state 4. */
int rsu_update_table_run_adam_clip(const void* dev_table, int nentries, int total_blocks, float alpha, float beta1, float beta2,
                                   float epsilon, float gscale, const void* state, rsu_stream_t stream);

/* ---- optimizer: moving average of the weights (new) -------- */
/* tf.train.ExponentialMovingAverage's assign_moving_average over ema[0, n) and w[0, n), per element, float32, in this order, no
 * contraction:
 *   ema[i] = ema[i] - (ema[i] - w[i]) * one_minus_decay
 * The caller computes one_minus_decay = 1 - decay_t in float32 (with TensorFlow's num_updates rule decay_t = min(decay, (1 + t) /
 * (10 + t))). ONE launch on `stream`, behind the update pass whose weights it averages: 256-lane workgroups over shares of 8192 floats,
 * a grid that depends on n ALONE -- not on the CU budget, the device or the autotuner. Reads ema and w once, writes ema: 12 B per
 * weight. Only ema[0, n) is written and only w[0, n) is read (the n & 3 scalars behind the last float4 singly).
 * clip_state: NULL, or the record rsu_grad_norm wrote earlier on the same stream. With RSU_CLIP_NONFINITE set in it every workgroup
 * returns before its first load, exactly as the _clip update passes do: a skipped step leaves weights, slots, packed copies AND
 * averages as they were. Any other record behaves as NULL (the scale is the gradient's business, not the average's).
 * Errors, returned before anything is launched: RSU_EINVAL for a NULL ema or w, n < 1, a one_minus_decay that is not in (0, 1] (nan
 * included), an ema or w that is not 16-byte aligned, overlapping ema and w ranges, a clip_state that is not 4-byte aligned. */
/* align (rsu_ema_step): ema 16, w 16, clip_state 4. */
int rsu_ema_step(float* ema, const float* w, long n, float one_minus_decay, const void* clip_state /* may be NULL */,
                 rsu_stream_t stream);

/* ---- optimizer: gradient accumulation over micro-batches (new) -------- */
/* dst[i] = assign ? src[i] : dst[i] + src[i] over [0, n), per element, float32, one rounding. What a host needs to take one optimizer
 * step over K backward passes, each of which OVERWRITES its gradient buffer g: with a second buffer gsum of the same size,
 *   pass 0:          rsu_grad_accumulate(gsum, g, n, 1)      gsum  = g_0            (whatever gsum held is forgotten, a nan included)
 *   pass 0 < j < K-1: rsu_grad_accumulate(gsum, g, n, 0)      gsum += g_j
 *   pass K-1:        rsu_grad_accumulate(g, gsum, n, 0)      g     = gsum + g_{K-1}
 * leaves ((g_0 + g_1) + ...) + g_{K-1} in g, where the exchange, rsu_grad_norm and the update tables read it (float32 addition
 * commutes, so the last line's operand order changes no bit). ONE launch on `stream`: 256-lane workgroups over shares of
 * RSU_GRAD_ACCUMULATE_BLOCK_FLOATS floats, a grid that depends on n ALONE -- not on the CU budget, the device or the autotuner. No
 * atomics, no LDS. assign == 0 reads dst and src once and writes dst: 12 B per element; assign != 0 does NOT read dst: 8 B per element.
 * Only dst[0, n) is written and only src[0, n) is read (the n & 3 scalars behind the last float4 singly). inf and nan pass through by
 * the IEEE rules and nothing is filtered: the non-finite guard of rsu_grad_norm sees them in the accumulated gradient.
 * Errors, returned before anything is launched: RSU_EINVAL for a NULL dst or src, n < 1, a dst or src that is not 16-byte aligned,
 * overlapping [dst, dst + n) and [src, src + n); RSU_E2BIG for an n whose grid would not fit 31 bits. */
#define RSU_GRAD_ACCUMULATE_BLOCK_FLOATS 8192
/* align (rsu_grad_accumulate): dst 16, src 16. */
int rsu_grad_accumulate(float* dst, const float* src, long n, int assign, rsu_stream_t stream);

/* ---- patch / stride tiler (src/images.py) -------------------------------------------------- */
/* images.py:269-281 mirror_border + :35-85 extract_patches fused, on device: tile t (x-outer,
 * y-inner order, images.py:76-77) of image n is the [S][S] window of the symmetric-padded image at
 * origin (x0, y0) = ((t / pps) * stride, (t % pps) * stride). imgs f32 [nimg][H][H][3];
 * tiles f32 [ntiles][S][S][3] for tile indices [t0, t0+ntiles) of the flattened (img, t) list. */
/* align (rsu_extract_tiles): imgs 4, tiles 4. */
int rsu_extract_tiles(const float* imgs, float* tiles, int nimg, int H, int S, int P, int stride, long t0,
                      long ntiles, rsu_stream_t stream);
/* images.py:131-164 images_from_patches, accumulation half: acc[n][y0+i][x0+j] += prob[t][i][j],
 * hits += 1 (f32 accumulators [nimg][H][H]; the division is rsu_overlap_finish). */
/* align (rsu_overlap_add): prob 4, acc 4, hits 4. */
int rsu_overlap_add(const float* prob, float* acc, float* hits, int nimg, int H, int P, int stride, long t0,
                    long ntiles, rsu_stream_t stream);
/* align (rsu_overlap_finish): acc 4, hits 4, out 4. */
int rsu_overlap_finish(const float* acc, const float* hits, float* out, long n, rsu_stream_t stream);

/* ---- the tiler for images of any size: rectangular, any stride, clamped last tile (new) ----- */
/* The tile grid of an H x W image. Along an axis of length L >= P with stride s >= 1 the tile origins are 0, s, 2s, ... while
 * o + P <= L; where (L - P) % s != 0 one more tile follows at L - P, the CLAMPED last tile, which overlaps its neighbour by more than
 * the others do. n = ceil((L - P) / s) + 1 tiles, the origin of tile i is min(i * s, L - P); an axis with (L - P) % s == 0 has exactly
 * the grid of rsu_extract_tiles. Tile order as there: image-major, then x (column) outer, y (row) inner, ny x nx tiles per image.
 * Host only. RSU_EINVAL for a NULL ny or nx, P < 1, P > H, P > W, stride < 1. */
int rsu_tile_grid(int H, int W, int P, int stride, int* ny, int* nx);
/* rsu_extract_tiles on that grid. imgs f32 [nimg][H][W][3]; tiles f32 [ntiles][S][S][3] for the tile indices [t0, t0 + ntiles) of the
 * flattened (img, x index, y index) list. The mirror border (S - P) / 2 is np.pad(..., "symmetric") of ANY width: the source index of
 * coordinate c along an axis of length L is m < L ? m : 2L - 1 - m with m = c mod 2L (non-negative), so a border wider than the image
 * reflects repeatedly. Pure data movement; every index is 64-bit. On an input rsu_extract_tiles accepts the tiles are its tiles.
 * Errors, returned before anything is launched: RSU_EINVAL for a NULL imgs or tiles, nimg < 1, P > H, P > W, P > S, an odd S - P,
 * stride < 1, t0 < 0, ntiles < 1, t0 + ntiles > nimg * nx * ny. */
/* align (rsu_extract_tiles_rect): imgs 4, tiles 4. */
int rsu_extract_tiles_rect(const float* imgs, float* tiles, int nimg, int H, int W, int S, int P, int stride, long t0,
                           long ntiles, rsu_stream_t stream);
/* rsu_overlap_add on that grid: acc and hits f32 [nimg][H][W]. Gather form, one thread per output pixel, no atomics: the pixel's
 * covering tiles of [t0, t0 + ntiles) are summed in increasing tile index (per axis the regular tiles, then the clamped one, each
 * counted once) in double and added to acc once per call; hits += their number. On an input rsu_overlap_add accepts acc and hits get
 * its bits. The division is rsu_overlap_finish. Errors as rsu_extract_tiles_rect (without S), for a NULL prob, acc or hits. */
/* align (rsu_overlap_add_rect): prob 4, acc 4, hits 4. */
int rsu_overlap_add_rect(const float* prob, float* acc, float* hits, int nimg, int H, int W, int P, int stride, long t0,
                         long ntiles, rsu_stream_t stream);

/* ---- training input: one launch per batch, with rotation and scale (new) -------------------- */
/* Cuts the input windows and label patches of a batch out of the resident training images, each sample through a 2x2 matrix of its own
 * about its window's centre. images f32 [nimg][He][He][3]: the mirror-extended images of the patch pool; labels uint8 [nimg][Hl][Hl] in
 * {0, 1}; offset = (He - Hl) / 2 = (S - P) / 2 (both differences even). recs: nrec records in HOST memory, read before the call returns;
 * x_out f32 [nrec][S][S][3]; labels_out int64 [nrec][P][P].
 * Record r: `image` in [0, nimg); (cy, cx) the centre of the window in the EXTENDED image's pixel coordinates, row and column (the pool's
 * patch at (x0, y0): cy = y0 + (S - 1) / 2, cx = x0 + (S - 1) / 2); M = [[m00, m01], [m10, m11]] maps an output offset (rows, columns)
 * to a source offset. Input pixel (i, j), all arithmetic float32, every operation rounded on its own, in this order:
 *   di = i - (S - 1) / 2,  dj = j - (S - 1) / 2
 *   sy = (cy - offset) + (m00 * di + m01 * dj),  sx = (cx - offset) + (m10 * di + m11 * dj)      (the ORIGINAL image's frame)
 *   y0 = floorf(sy), fy = sy - y0; x0 = floorf(sx), fx = sx - x0; taps: rows y0, y0 + 1, columns x0, x0 + 1
 *   each tap index t reflected on its own into [0, Hl): m = ((t % 2Hl) + 2Hl) % 2Hl, index = m < Hl ? m : 2Hl - 1 - m (numpy's
 *   "symmetric" padding, images.py mirror_border, repeated as often as needed), then read at (index + offset) of the extended image
 *   value, per channel = (v00 * (1 - fx) + v01 * fx) * (1 - fy) + (v10 * (1 - fx) + v11 * fx) * fy      (v<row tap><column tap>)
 * With fx = fy = 0 this is the source pixel bit for bit (finite data; a -0.0 may come out as +0.0). Label pixel (i, j): the same with
 * (P - 1) / 2 in place of (S - 1) / 2, the uint8 labels read as floats and reflected in their own [Hl][Hl] frame; 1 where the
 * interpolated value is >= 0.5, else 0. Window and patch are concentric, and image and labels reflect about the same edges: a rotated
 * window never pairs mirrored pixels with unmirrored labels. The identity matrix gives the pool's plain window, the eight signed
 * permutation matrices its D4 symmetries, (1 / s) R(theta) a rotation by theta with zoom s. hostio.affine_patches restates the rule in
 * numpy float32: the outputs are reproducible bit for bit on the host.
 * The records travel as kernel arguments, RSU_AFFINE_MAX_LAUNCH per launch: ceil(nrec / 32) launches on `stream`, no device table, no
 * copy, no synchronisation, no allocation. A sample's output depends on its own record alone, not on its neighbours or on where the
 * record list is cut. Errors, returned before anything is launched or written: RSU_EINVAL for a NULL images, labels, recs, x_out or
 * labels_out, nrec, nimg, Hl or P below 1, S < P, He - Hl or S - P odd or different, an `image` outside [0, nimg), a record field that
 * is not finite, max |m| > 64 or a centre beyond +-2^22 (together they keep every coordinate far inside float32's exact-integer range);
 * RSU_E2BIG where one image or one output tensor reaches 2 GiB (the image base is 64-bit: the pool as a whole may exceed 2 GiB). */
typedef struct {
    int image;
    float cy, cx;
    float m00, m01, m10, m11;
    int pad_;
} rsu_affine_t; /* 32 bytes */
#define RSU_AFFINE_MAX_LAUNCH 32
/* align (rsu_affine_patches): images 4, labels byte, recs host, x_out 4, labels_out 8. */
int rsu_affine_patches(const float* images, const uint8_t* labels, const rsu_affine_t* recs /* HOST pointer */, int nrec, int nimg, int He,
                       int Hl, int S, int P, float* x_out, int64_t* labels_out, rsu_stream_t stream);

/* ---- training input: the same launch with an elastic deformation per sample (new) ------------ */
/* rsu_affine_patches with a smooth random displacement of every output pixel in front of the matrix: the U-Net paper's elastic deformation
 * (displacement vectors on a coarse grid, interpolated smoothly), formed per pixel inside the loader kernel -- no further copy of the
 * training set and no further pass over the batch. images, labels, nrec, nimg, He, Hl, S, P, offset, x_out, labels_out and the record
 * fields image, cy, cx, m00 .. m11 are rsu_affine_patches'. Further fields of record r: alpha >= 0, the standard deviation of the CONTROL
 * POINTS in OUTPUT pixels (the interpolated field's deviation is smaller: a cubic B-spline averages its 16 neighbours); key, the key of the
 * sample's lattice; grid = G, the lattice's cells per axis across the input window, 1 .. RSU_ELASTIC_MAX_GRID. The padding is not read.
 * All arithmetic float32, every operation rounded on its own, in this order:
 *   lattice  (G + 3) x (G + 3) control points of two components, stored nowhere. Component `axis` (0 = rows, 1 = columns) of point (a, b),
 *            0 <= a, b < G + 3, is c_axis[a][b] = alpha * g with g the noise value of rsu_color_jitter below for the element index
 *            e = (a * 32 + b) * 2 + axis under `key`: h1 = mix(e ^ key), h2 = mix(h1 ^ 0x9e3779b9), n = the sum of their four 16-bit halves,
 *            g = ((float)n - 131070.f) * C with that entry's C. |g| <= 131070 C < 3.4641. The key is XORed in: keys must be uniform 32-bit
 *            draws (pool.elastic_draw), keys that differ in low bits only give permuted copies of one lattice.
 *   cell     per axis, for the INPUT WINDOW's pixel index iw in [0, S): q = (float)((double)G / (double)S), formed on the host inside the
 *            call and passed to the kernel (the device never divides);
 *              t = ((float)iw + 0.5f) * q,  k = (int)floorf(t) clamped to [0, G - 1],  f = t - (float)k
 *   weights  of the uniform cubic B-spline, with g1 = 1.0f - f, f2 = f * f, f3 = f2 * f and SIXTH = the float with bits 0x3e2aaaab (1 / 6
 *            rounded; a product, not a quotient):
 *              w[0] = ((g1 * g1) * g1) * SIXTH                              (1 - f)^3 / 6
 *              w[1] = ((3.0f * f3 - 6.0f * f2) + 4.0f) * SIXTH              (3 f^3 - 6 f^2 + 4) / 6
 *              w[2] = (((3.0f * f2 - 3.0f * f3) + 3.0f * f) + 1.0f) * SIXTH (-3 f^3 + 3 f^2 + 3 f + 1) / 6
 *              w[3] = f3 * SIXTH                                            f^3 / 6
 *            (ky, wy[]) from the row index, (kx, wx[]) from the column index
 *   field    row_a  = ((wx[0] * c_axis[ky + a][kx] + wx[1] * c_axis[ky + a][kx + 1]) + wx[2] * c_axis[ky + a][kx + 2]) + wx[3] * c_axis[ky + a][kx + 3]
 *            u_axis = ((wy[0] * row_0 + wy[1] * row_1) + wy[2] * row_2) + wy[3] * row_3
 *            The weights are a partition of unity up to rounding (their sum is within 2^-22 of 1), so |u| <= 3.47 alpha.
 *   use      input pixel (i, j): iw = i, jw = j; di = (i - (S - 1) / 2) + u_0, dj = (j - (S - 1) / 2) + u_1; everything behind that is
 *            rsu_affine_patches from "sy =" on, unchanged: M, the centre, floor and fractions, every tap reflected on its own about the
 *            ORIGINAL image's edges, the interpolation. The displacement is an OUTPUT offset: it rotates and zooms with the sample.
 *            Label pixel (i, j): iw = i + offset, jw = j + offset -- its own pixel of the window -- and (P - 1) / 2 in place of
 *            (S - 1) / 2: the same float operations on the same integers (i - (P - 1) / 2 and (i + offset) - (S - 1) / 2 are the same
 *            float), so a label is displaced by exactly the field its window pixel sees.
 * alpha = 0 gives c = +-0 and u = +-0: di and dj keep their bits and the sample equals rsu_affine_patches' bit for bit. A large alpha on a
 * fine grid (alpha above about S / (3 G)) can FOLD the field -- neighbouring output pixels read the source in reversed order; nothing here
 * prevents it, the choice is the caller's. hostio.elastic_patches restates the rule in numpy float32: the outputs are reproducible bit for
 * bit on the host. The records travel as kernel arguments, RSU_ELASTIC_MAX_LAUNCH per launch (1.5 KB): ceil(nrec / 32) launches on
 * `stream`, no device table, no copy, no synchronisation, no allocation. A sample's output depends on its own record alone, not on its
 * neighbours or on where the record list is cut. Errors, returned before anything is launched or written: everything rsu_affine_patches
 * refuses, with the same codes; RSU_EINVAL for an alpha that is not finite, negative or above 64, a grid outside [1, RSU_ELASTIC_MAX_GRID]. */
typedef struct {
    int image;
    float cy, cx;
    float m00, m01, m10, m11;
    float alpha;   /* standard deviation of the control points, in output pixels, >= 0 */
    unsigned key;  /* key of this sample's lattice */
    int grid;      /* G: cells per axis across the input window */
    int pad_[2];
} rsu_elastic_t; /* 48 bytes */
#define RSU_ELASTIC_MAX_LAUNCH 32
#define RSU_ELASTIC_MAX_GRID 16
/* align (rsu_elastic_patches): images 4, labels byte, recs host, x_out 4, labels_out 8. */
int rsu_elastic_patches(const float* images, const uint8_t* labels, const rsu_elastic_t* recs /* HOST pointer */, int nrec, int nimg, int He,
                        int Hl, int S, int P, float* x_out, int64_t* labels_out, rsu_stream_t stream);

/* ---- training input: colour jitter and noise per sample, behind the loader (new) ------------- */
/* Photometric augmentation of a finished batch, in place: sample n of x f32 [nrec][S][S][3] is transformed by record n alone. recs: nrec
 * records in HOST memory, read before the call returns. Pixel p = i * S + j of a sample has channels x0, x1, x2. All arithmetic is
 * float32, every operation rounded on its own, in the order written:
 *   means   skipped when all nine k[] of the record are zero: then m = 0 and ws is never read for the sample. Otherwise, with
 *             q(v)  = (int64) rintf(fminf(fmaxf(v, -256.f), 256.f) * 16777216.f)
 *             sum_c = the exact int64 sum of q(x_c) over the sample's S * S pixels
 *             m_c   = (float)((double)sum_c / ((double)(S * S) * 16777216.0))
 *           (integer sums: the result does not depend on the order of summation, so the kernel is free in how it cuts the work, and the
 *           host restates it with np.rint and an int64 sum)
 *   colour  d_r = (k[3r] * m0 + k[3r+1] * m1) + k[3r+2] * m2
 *           y_r = ((a[3r] * x0 + a[3r+1] * x1) + a[3r+2] * x2) + d_r
 *   noise   only when sigma > 0. Element index e = 3 * p + r as unsigned; mix(v): v ^= v >> 16; v *= 0x85ebca6b; v ^= v >> 13;
 *           v *= 0xc2b2ae35; v ^= v >> 16 (the finaliser the dropout hash uses);
 *             h1 = mix(e ^ key), h2 = mix(h1 ^ 0x9e3779b9)
 *             n  = (h1 & 0xffff) + (h1 >> 16) + (h2 & 0xffff) + (h2 >> 16)     an Irwin-Hall sum of four 16-bit uniforms: mean 131070,
 *                                                                              standard deviation sqrt((65536^2 - 1) / 3) = 37837.227...
 *             g  = ((float)n - 131070.f) * C,  C = the float with bits 0x37ddb3d7 (1 / 37837.227...)
 *             y_r = y_r + sigma * g
 *   clamp   out_r = fminf(fmaxf(y_r, 0.f), 1.f)      (a -0.0 may come out as +0.0)
 * The identity record (A = I, K = 0, sigma = 0) returns data in [0, 1] bit for bit. With A = c b H Sat and K = (1 - c) b H Sat this is
 * brightness b, contrast c about the sample's own per-channel mean (tf.image.adjust_contrast), saturation and hue in one pass
 * (pool.jitter_draw). hostio.color_jitter restates the rule in numpy float32: the output is reproducible bit for bit on the host.
 * Launches on `stream`, per RSU_JITTER_MAX_LAUNCH records (they travel as kernel arguments): one that sums (only when a record of the
 * launch has a non-zero k[]) and one that applies; no memset, copy, allocation, atomics or synchronisation. ws: rsu_color_jitter_ws_bytes(nrec,
 * S) bytes (0 for nrec or S below 1), 8-byte aligned: three int64 partial sums per 4096-pixel share of a sample, for the records of one
 * launch -- every launch of a call re-uses it, stream order keeps them apart -- written before they are read, nothing to zero: it need not be
 * cleared and holds nothing between calls. A
 * sample's output depends on its own record alone, not on its neighbours or on where the record list is cut.
 * Errors, returned before anything is launched or written: RSU_EINVAL for a NULL x or recs, nrec or S below 1, a record field that is
 * not finite, |a| or |k| above 64, sigma outside [0, 1], a NULL ws while some record has a non-zero k[], a ws that is not 8-byte aligned;
 * RSU_E2BIG where x reaches 2 GiB. */
typedef struct {
    float a[9];    /* A, row-major: output channel r, input channel k at a[3r + k] */
    float k[9];    /* K, likewise: the weight of the sample's channel means */
    float sigma;   /* noise amplitude, >= 0 */
    unsigned key;  /* noise key */
} rsu_jitter_t;    /* 80 bytes */
#define RSU_JITTER_MAX_LAUNCH 32
size_t rsu_color_jitter_ws_bytes(int nrec, int S);
/* align (rsu_color_jitter): x 4, recs host, ws 8. */
int rsu_color_jitter(float* x /* f32 [nrec][S][S][3], in place */, const rsu_jitter_t* recs /* HOST pointer */,
                     int nrec, int S, void* ws /* may be NULL when every k[] is zero */, rsu_stream_t stream);

/* ---- post-processing wire format (src/images.py) and metric counters (src/summary.py) ------ */
/* images.py:256-266 quantize_mask: per patch_size block of masks f32 [nimg][S][S] (channel axis squeezed), label =
 * mean(mask >= 0.5) > threshold, written over the block of `out` (out == masks is allowed: a block is read completely before it
 * is written). patch_size <= 64. */
/* align (rsu_quantize_mask): masks 4, out 4. */
int rsu_quantize_mask(const float* masks, float* out, int nimg, int S, int patch_size, float threshold, rsu_stream_t stream);
/* rsu_quantize_mask on masks f32 [nimg][H][W]: the same rule per patch_size block; a block cut by the image's edge takes the mean over
 * the pixels it holds. out == masks is allowed; patch_size <= 64. RSU_EINVAL for a NULL masks or out, nimg, H, W or patch_size below 1,
 * patch_size above 64; RSU_E2BIG for more than 2^31 - 1 blocks. */
/* align (rsu_quantize_mask_rect): masks 4, out 4. */
int rsu_quantize_mask_rect(const float* masks, float* out, int nimg, int H, int W, int patch_size, float threshold,
                           rsu_stream_t stream);
/* images.py:88-99 labels_for_patches over images.py:35-85 extract_patches(masks, patch_size): labels int64
 * [nimg][S/ps][S/ps] in the reference's patch order (x outer, y inner), label = mean(patch) > threshold. */
/* align (rsu_labels_for_patches): masks 4, labels 8. */
int rsu_labels_for_patches(const float* masks, int64_t* labels, int nimg, int S, int patch_size, float threshold,
                           rsu_stream_t stream);
/* summary.py:141-147 tf.metrics.accuracy / recall / precision keep running counts: counts[0..3] += TP, FP, FN, TN of n
 * int64 {0,1} labels (caller zeroes `counts` where the reference runs tf.local_variables_initializer()). */
/* align (rsu_confusion_counts): predictions 8, labels 8, counts 8. */
int rsu_confusion_counts(const int64_t* predictions, const int64_t* labels, long n, unsigned long long* counts,
                         rsu_stream_t stream);

/* ---- static shape table (tf_aerial_images.py:133-145 build_graph fixes every shape up front) ---------- */
#define RSU_OP_COLOR_ADJUST 0 /* unet.py:22-23 */
#define RSU_OP_CONV3X3 1      /* unet.py:34-45, 88-91 (dilation 1 or 2; nsrc > 1: virtually concatenated crops) */
#define RSU_OP_MAXPOOL 2      /* unet.py:52 */
#define RSU_OP_CONVT2X2 3     /* unet.py:67-68 */
#define RSU_OP_HEAD 4         /* unet.py:95 + tf_aerial_images.py:147-148 */
typedef struct {
    int kind, level;          /* RSU_OP_*; block index as in the reference's scope names (conv_<level>) */
    int Hin, Win, Cin;        /* input window (of every source) and total input channels */
    int Hout, Wout, Cout;
    int dilation, nsrc;
} rsu_plan_row_t;
typedef struct {
    int input_size;           /* unet.input_size_needed(patch_size, num_layers) */
    long num_params;          /* every variable unet.forward creates (the dead level L-1 dilated pair included) */
    long activation_elems;    /* bf16 elements of all op outputs for `batch` patches */
    size_t workspace_floats;  /* largest scratch any backward entry point of this network asks for */
} rsu_plan_totals_t;
/* Ops of unet.forward in execution order for a (num_layers, root_size, patch_size, dilated) network: a binder needs no shape
 * arithmetic of its own. rows may be NULL (count only); RSU_ENOMEM when capacity is too small (nrows still set). */
int rsu_plan(int num_layers, int root_size, int patch_size, int dilated, int batch, rsu_plan_row_t* rows, int capacity,
             int* nrows, rsu_plan_totals_t* totals);

#ifdef __cplusplus
}
#endif
#endif /* RSU_H_ */
