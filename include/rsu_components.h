/*
 * rsu_components.h -- the sixth public header of librsu_hip.so: connected components of binary masks on the device -- labelling, the
 * clean-up of a predicted mask (small components removed, small holes filled) and a connectivity count for validation.
 *
 * Same library, same conventions and memory contract as rsu.h (plain C, device pointers + sizes, `stream` a hipStream_t passed as void*,
 * asynchronous on that stream, 0 on success and a negative RSU_E* code otherwise). tests/test_gpu_components_fenced.py holds every
 * launching entry of this header to the memory contract; road_segmentation_unet_amd/_lib.py binds it through its table
 * SIGNATURES_COMPONENTS.
 */
#ifndef RSU_COMPONENTS_H_
#define RSU_COMPONENTS_H_

#include "rsu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- connected components (new; the reference has none, torch has no such operator) -------------------------------------------- */
/* Shared by all entries. prob is float32 [N][H][W] (what the heads and predict() write).
 *   images:       independent. No label, count or link crosses from one image into another.
 *   foreground:   a pixel is foreground iff p >= threshold: one float32 comparison, the only float operation of this header. NaN is
 *                 background, p == threshold is foreground (the rule of rsu_quantize_mask and of the evaluation's counts).
 *   connectivity: 4 (edge neighbours) or 8 (edge and corner neighbours). The DUAL connectivity is 4 for 8 and 8 for 4.
 *   labels:       a component's label is 1 + the smallest row-major index y * W + x among its pixels; background is 0. A property of the
 *                 mask alone: no result depends on the grid, the wave order, the order of atomics or the tiling.
 *   limits:       N, H, W >= 1, H * W <= 2^24, N * H * W < 2^31; threshold finite; connectivity 4 or 8; min_area, max_hole >= 0.
 *                 RSU_EINVAL otherwise and for a NULL required pointer, before anything is launched or written.
 *
 * The method. Tiles of 64 x 64 pixels; tiles_y = ceil(H / 64), tiles_x = ceil(W / 64), M = ceil(log2(max(tiles_y, tiles_x))) (0 for one
 * tile). One LABELLING is 2 + M launches: one workgroup per tile runs a union-find over the tile in LDS; at level m = 1 .. M one workgroup
 * per 2^m x 2^m group of tiles unites the pixel pairs across the group's two new inner borders, so that the sets two workgroups of a launch
 * touch are disjoint (the L2s of the chip's dies need not agree inside a launch); a flatten launch walks every pixel to its root, and
 * every tile-level root adds its tile's area to its component's total and ORs its edge flag in (one integer atomic pair per tile-level
 * component, never one per pixel). The larger root is always linked under the smaller (an integer atomic min), so parents only decrease:
 * every data-dependent loop ends by that alone. No grid-wide barrier, no cooperative launch, no flag or wait between workgroups, no float
 * atomic; the integer atomics used (min, add, or) do not depend on their order. The launch counts below depend on N, H, W and the arguments
 * alone, never on the data. No host synchronisation, no allocation.
 *
 * ws: rsu_components_ws_bytes bytes, 4-byte aligned, one size for all three entries: five int32 arrays of N * H * W elements (parents;
 * labels and per-pixel totals of the filter's two labellings) and four int32 counters per image: 20 * N * H * W + 16 * N bytes. It need
 * not be cleared and holds nothing between calls. */
size_t rsu_components_ws_bytes(int N, int H, int W);   /* 0 for refused sizes */

/* rsu_components_label: invert == 0 labels the foreground, invert != 0 the complement (the pixels that are not foreground, NaN included).
 * labels int32 [N][H][W] as defined above. area int32 [N][H][W] (may be NULL): at every labelled pixel the pixel count of its component,
 * 0 elsewhere. edge uint8 [N][H][W] (may be NULL): 1 at every labelled pixel whose component has a pixel in row 0, row H - 1, column 0 or
 * column W - 1, 0 elsewhere. Launches: 2 + M, and one more when area or edge is given. Nothing is written outside labels, area, edge, ws. */
/* align (rsu_components_label): prob 4, labels 4, area 4, edge byte, ws 4. */
int rsu_components_label(const float* prob, float threshold, int connectivity, int invert, int32_t* labels, int32_t* area, uint8_t* edge,
                         void* ws, int N, int H, int W, rsu_stream_t stream);

/* rsu_components_filter: the clean-up of a predicted mask, in this fixed order:
 *   1. F0 = {p >= threshold}; its components at `connectivity`; those with area < min_area are REMOVED. min_area <= 1 removes nothing,
 *      and this labelling is not launched. F1 = F0 minus the removed pixels.
 *   2. the complement of F1 (removed pixels and NaN pixels included); its components at the DUAL connectivity. A HOLE is such a component
 *      with edge == 0; holes with area <= max_hole are FILLED. max_hole == 0 fills nothing, and this labelling is not launched.
 *   3. out[p] (float32 [N][H][W]; out == prob is allowed): 1.0f at a filled pixel, also one that step 1 removed; +0.0f at a removed pixel
 *      that was not filled; the bits of prob[p] otherwise (NaN payloads included).
 *   4. stats int64 [N][6] (may be NULL), written, not accumulated: {components of F0, components removed, pixels removed, holes, holes
 *      filled, pixels filled} of image n. A skipped labelling writes its three fields as 0.
 * Launches: (2 + M) * (labellings not skipped) + 1. Nothing is written outside out, stats and ws. */
/* align (rsu_components_filter): prob 4, out 4, stats 8, ws 4. */
int rsu_components_filter(const float* prob, float threshold, int connectivity, int min_area, int max_hole, float* out, int64_t* stats,
                          void* ws, int N, int H, int W, rsu_stream_t stream);

/* rsu_components_pair_count: a connectivity figure for validation. labels64 int64 [N][H][W]; a pixel is COUNTED iff its label is 0 or 1
 * (all 64 bits tested, as in the heads). Per image: cp = the components of {counted and p >= threshold}, cy = the components of
 * {label == 1}, both at `connectivity`; ignored pixels are background in both. acc (4 unsigned 64-bit integers, accumulated: the caller
 * zeroes them): acc[0] += sum cp, acc[1] += sum cy, acc[2] += sum |cp - cy|, acc[3] += the images with at least one counted pixel. An
 * image without a counted pixel (the padding of an evaluation chunk: labels -1) adds exactly nothing. Both masks of every image are
 * labelled by the same launches: 3 + M in all. Nothing is written outside acc[0..3] and ws. */
/* align (rsu_components_pair_count): prob 4, labels64 8, acc 8, ws 4. */
int rsu_components_pair_count(const float* prob, float threshold, const int64_t* labels64, int connectivity, unsigned long long* acc, void* ws,
                              int N, int H, int W, rsu_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RSU_COMPONENTS_H_ */
