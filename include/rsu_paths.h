/*
 * rsu_paths.h -- the eleventh public header of librsu_hip.so: the fourth step from a mask to a road network. It orders the pixels of
 * every road segment of rsu_segments.h along the segment, on the device, so that an edge of the network has a geometry: a polyline that
 * can be drawn, exported, simplified, resampled or compared point by point. It reads the outputs of one rsu_line_segments call, so the
 * chain thin -> prune -> segments -> paths never leaves the device.
 *
 * Same library, same conventions and memory contract as rsu.h (plain C, device pointers + sizes, `stream` a hipStream_t passed as
 * void*, asynchronous on that stream, 0 on success and a negative RSU_E* code otherwise, returned before anything is launched or
 * dereferenced; no allocation, no host synchronisation). tests/test_gpu_paths_fenced.py holds the launching entry of this header to the
 * memory contract; road_segmentation_unet_amd/_lib.py binds it through its table SIGNATURES_PATHS.
 */
#ifndef RSU_PATHS_H_
#define RSU_PATHS_H_

#include "rsu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- ordered polylines of road segments (new; the reference has none) -------------------------------------------------------------- */
/* Inputs. They come from one rsu_line_segments call, for one side per call:
 *   seg:    int32 [N][H][W], seg_pred or seg_true: the segment label at segment pixels, 0 elsewhere.
 *   edges:  int32 [N][max_edges][8], that side's rows {label, pixels, ...} in ascending label order.
 *   counts: int32 [N][4]. side 0 reads counts[n][0], side 1 reads counts[n][2].
 *   stored = min(count, max_edges) rows are read. Pixels whose label has no stored row are skipped.
 *   images: independent. Everything outside an image is background.
 *
 * Path links. S = {seg != 0}. Two pixels of S are linked iff
 *   - they are 4-adjacent, or
 *   - they are diagonal neighbours and neither of the two pixels 4-adjacent to both is in S.
 * This is rsu_segments.h's link rule with S in place of A. With it the link graph of every 8-connected segment is connected, and a
 * segment without a pixel of link degree 3 or more is a single pixel, a chain with exactly two terminals, or a cycle with none.
 *
 * Kind of a stored row, tested in this order:
 *   3 (too long):  the row's `pixels` is greater than max_len.
 *   2 (branched):  some pixel of it has link degree 3 or more.
 *   0 (open):      otherwise, if it has a pixel of link degree 1 or less (there are then exactly two, or the segment is one pixel).
 *   1 (ring):      otherwise.
 *
 * Order.
 *   open: position 0 is the terminal with the smaller row-major index; positions follow the links.
 *   ring: position 0 is the pixel with the smallest index (label - 1), position 1 the smaller-indexed of its two link neighbours, then
 *         on round.
 *   Kinds 2 and 3 are not ordered and store no point.
 *
 * The method. Pointer jumping over arcs: a chain has no orientation, so every segment pixel owns up to two arcs (pixel, slot) towards
 * its link neighbours in ascending index; the successor of the arc v -> w is w's other arc; an arc whose head is a terminal of an open
 * segment or the smallest pixel of a ring is final. An arc holds one 64-bit word {arc reached, hops}; one doubling is
 * J[a] = {J[J[a].arc].arc, J[a].hops + J[J[a].arc].hops}; a pixel's position is hops + 1 of its arc whose final arc enters the start pixel
 * (for a ring: and leaves from the start's smaller neighbour). A segment of n pixels needs at most n - 2 hops, so
 * R = ceil(log2(max_len)) doublings suffice. The launches: one that resets the per-row minima, flags and the per-image counters in ws; a
 * classify launch (link masks from a tile with a one-pixel halo in LDS, each label's row by binary search over the ascending labels, the
 * rows' terminal minimum and branched flag by integer min / or atomics: order-free); one workgroup per image for kinds, the scan and
 * info; an arc launch; R jump launches, one doubling each, reading one arc buffer and writing the other, so that no workgroup reads
 * within a launch what another wrote in it; an emit launch. A jump launch counts its changed arcs per image (one integer atomic per
 * workgroup of 2048 pixels); the next one returns at once for an image whose count is 0. The launch count,
 *     5 + R,
 * is fixed by max_len; no float operation, no flag between workgroups, no grid-wide barrier, no float atomic.
 *
 * The kernels (gfx950, 256 threads each, no scratch; from the build's ISA):
 *     k_paths_init     14 VGPRs,    0 bytes of LDS, 8 waves per SIMD
 *     k_paths_classify 24 VGPRs, 4752 bytes of LDS, 8 waves per SIMD
 *     k_paths_rows     20 VGPRs, 1036 bytes of LDS, 8 waves per SIMD
 *     k_paths_arcs     18 VGPRs,    0 bytes of LDS, 8 waves per SIMD
 *     k_paths_jump     16 VGPRs,    4 bytes of LDS, 8 waves per SIMD
 *     k_paths_emit      8 VGPRs,    0 bytes of LDS, 8 waves per SIMD
 *
 * ws: rsu_paths_ws_bytes bytes, 8-byte aligned: two arc buffers of 16 N H W bytes each, one int32 plane [N][H][W], two int32 arrays
 * [N][max_edges], then int32 [max(R, 1)][N], rounded up to 8. It need not be cleared and holds nothing between calls. */
#define RSU_PATHS_MAX_SIDE 1024
#define RSU_PATHS_MAX_EDGES 65536
#define RSU_PATHS_MAX_LEN (1 << 20)
size_t rsu_paths_ws_bytes(int N, int H, int W, int max_edges, int max_len);   /* 0 for refused sizes */

/* offsets: int32 [N][max_edges + 1]: offsets[n][0 .. stored] are written, the exclusive sums of `pixels` over the stored rows of kind 0
 *      or 1. These are the true numbers, also past max_points.
 * paths: int32 [N][max_points]: paths[n][offsets[n][r] + p] is the row-major index y W + x of the pixel at position p of row r. An
 *      element at or past max_points is not written, nor is one that no ordered row owns.
 * kind: int32 [N][max_edges]: rows at and past stored are not touched.
 * pos: int32 [N][H][W], may be NULL: 1 + position at the pixels of ordered stored rows, 0 elsewhere.
 * info: int32 [N][4] = {offsets[n][stored], open rows, ring rows, rows of kind 2 or 3}, written. An image with stored == 0 writes four
 *      zeros.
 * No overlap between any two buffers is allowed. Every index formed from seg, edges and counts is range-checked before it addresses
 * memory: inconsistent inputs give unspecified values, never a write outside the outputs and ws.
 * RSU_EINVAL: N, H or W below 1; a side above RSU_PATHS_MAX_SIDE; `side` not 0 or 1; max_edges outside [1, RSU_PATHS_MAX_EDGES]; max_len
 *      outside [1, RSU_PATHS_MAX_LEN]; max_points outside [1, H W]; a NULL pointer other than pos.
 * RSU_E2BIG: the entry's largest internal array (one arc buffer, 16 N H W bytes) reaches 0x7ffffff0. At 1024 x 1024 the last admitted
 *      batch is 127 images, and 128 is refused.
 * An argument error is reported before the size. Nothing is written outside the outputs and ws. */
/* align (rsu_segment_paths): seg 4, edges 4, counts 4, paths 4, offsets 4, kind 4, pos 4, info 4, ws 8. */
int rsu_segment_paths(const int32_t* seg, const int32_t* edges, const int32_t* counts, int side, int max_edges, int max_len,
                      int max_points, int32_t* paths, int32_t* offsets, int32_t* kind, int32_t* pos, int32_t* info,
                      void* ws, int N, int H, int W, rsu_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RSU_PATHS_H_ */
