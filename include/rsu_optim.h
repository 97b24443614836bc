/*
 * rsu_optim.h -- the second public header of librsu_hip.so: optimizer entries added behind rsu.h (weight decay inside the update pass).
 *
 * Same library, same conventions and memory contract as rsu.h (plain C, device pointers + sizes, `stream` a hipStream_t passed as void*,
 * asynchronous on that stream, 0 on success and a negative RSU_E* code otherwise). tests/test_gpu_optim_fenced.py holds every launching
 * entry of this header to the memory contract, as tests/test_gpu_fenced.py does for rsu.h; road_segmentation_unet_amd/_lib.py binds it
 * through its table SIGNATURES_OPTIM.
 */
#ifndef RSU_OPTIM_H_
#define RSU_OPTIM_H_

#include "rsu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- optimizer: weight decay inside the update pass (new; the reference has none) -------- */
/* rsu_update_table_run / rsu_update_table_run_adam (rsu.h) with a decay step in front of the rule, in the SAME launch: the same device
 * table (rsu_update_table_add[_plain], rsu_update_table_set_second_slot, rsu_update_table_finish; a table built for the plain run is
 * valid here), the same grid of total_blocks workgroups, the same loads and stores per weight (24 B per weight of a packed kernel under
 * Momentum, 32 B under Adam).
 * What decays: the entries of rsu_update_table_add (3x3 conv kernels, the first conv, transposed-conv kernels). The plain ranges of
 * rsu_update_table_add_plain (biases, the colour-adjust matrix, the 1x1 head) run the plain rule. The zero padding of the packed
 * buffers is not written, as in the plain run.
 * Per element of a decaying entry, float32, every operation rounded on its own (no contraction), in this order:
 *   RSU_DECAY_DECOUPLED  w1 = w - (decay * w); then the entry's rule on (w1, slots, g), the code of the plain pass. The caller passes
 *                        decay = (float)lr_t * (float)lambda -- lr_t the scheduled rate, not Adam's bias-corrected alpha (AdamW; under
 *                        Momentum the same step in front of the Momentum rule).
 *   RSU_DECAY_L2         g1 = (gscale' * g) + (decay * w), decay = lambda: the gradient of the penalty lambda / 2 |w|^2; then the rule
 *                        with g1 where it used gscale' * g. The decay term is not clipped (rsu_grad_norm measures the data gradient only).
 * The packed copies are written from the new weights, with the bits of rsu_pack_*.
 * clip_state: NULL -- gscale' = gscale, the plain run with decay; or the record rsu_grad_norm wrote earlier on the same stream --
 * gscale' = gscale * state->scale, one float32 multiply per workgroup, as in the _clip runs; with RSU_CLIP_NONFINITE set in it every
 * workgroup returns before its first load: nothing moves, so a skipped step decays nothing either.
 * Errors, returned before anything is launched: RSU_EINVAL for whatever the plain run rejects, a decay that is not finite or not > 0, a
 * mode other than the two constants, a clip_state that is not 4-byte aligned. */
#define RSU_DECAY_L2 0
#define RSU_DECAY_DECOUPLED 1
/* align (rsu_update_table_run_decay): dev_table 8, clip_state 4. */
int rsu_update_table_run_decay(const void* dev_table, int nentries, int total_blocks, float lr, float mu, float gscale, float decay,
                               int mode, const void* clip_state /* may be NULL */, rsu_stream_t stream);
/* align (rsu_update_table_run_adam_decay): dev_table 8, clip_state 4. */
int rsu_update_table_run_adam_decay(const void* dev_table, int nentries, int total_blocks, float alpha, float beta1, float beta2,
                                    float epsilon, float gscale, float decay, int mode, const void* clip_state /* may be NULL */,
                                    rsu_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RSU_OPTIM_H_ */
