/*
 * rsu_segments.h -- the tenth public header of librsu_hip.so: the third step from a mask to a road network. It cuts a centre-line at
 * its junctions into road segments on the device and measures every one of them: which pixels form it, how long it is (orthogonal
 * and diagonal links, counted apart) and which two nodes it joins. It reads the formats of rsu_thin.h and rsu_graph.h, so the chain
 * thin -> prune -> segments never leaves the device; the caller gets the network as a vector output, one row of integers per segment.
 *
 * Same library, same conventions and memory contract as rsu.h (plain C, device pointers + sizes, `stream` a hipStream_t passed as
 * void*, asynchronous on that stream, 0 on success and a negative RSU_E* code otherwise, returned before anything is launched or
 * dereferenced; no allocation, no host synchronisation). tests/test_gpu_segments_fenced.py holds the launching entry of this header to
 * the memory contract; road_segmentation_unet_amd/_lib.py binds it through its table SIGNATURES_SEGMENTS.
 */
#ifndef RSU_SEGMENTS_H_
#define RSU_SEGMENTS_H_

#include "rsu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- road segments (new; the reference has none) ---------------------------------------------------------------------------------- */
/* prob is float32 [N][H][W], labels64 int64 [N][H][W].
 *
 * Masks. prob, threshold, labels64, "counted", P, T and image independence are rsu_graph.h's, word for word:
 *   images:   independent. Everything outside an image is background.
 *   counted:  a pixel is COUNTED iff its labels64 value is 0 or 1 (all 64 bits tested).
 *   P:        {counted and prob >= threshold}: one float32 comparison, the only float operation of this header. NaN is outside P,
 *             p == threshold is inside.
 *   T:        {labels64 == 1}. Ignored pixels are background on both sides.
 *   - The entry takes the two outputs of rsu_skeleton_graph (or of rsu_mask_thin) as they are.
 *   - It is defined on any mask all the same.
 *   - A stands for either mask.
 *
 * Junction pixels and node zones.
 *   - J = the pixels of A with crossing number X >= 3 (rsu_graph.h's X).
 *   - Z = A and dilate8(J), the 3 x 3 dilation with J itself included.
 *   - A NODE is an 8-connected component of Z. Its id is 1 + the smallest row-major index of its pixels (rsu_components.h's label).
 *   - Why not J alone: the first pixels of a T's three branches are diagonal neighbours of each other, so removing only J leaves the
 *     branches in one component. On the thinned bank of tests/thin_util.py about 30 % of the components of A \ J touch four or more
 *     nodes. With Z, more than 98 % touch exactly two.
 *
 * Segments.
 *   - S = A \ Z.
 *   - A SEGMENT is an 8-connected component of S.
 *   - Its label is 1 + its smallest row-major index.
 *
 * Per-segment measurements. All are integers.
 *   - pixels: its pixel count.
 *   - Links inside the segment. Each unordered pair of 8-adjacent pixels of the segment counts once.
 *       - An orthogonal pair adds 1 to ortho.
 *       - A diagonal pair adds 1 to diag only if neither of the two pixels that are 4-adjacent to both is in A. An L-corner is then two
 *         orthogonal links, not three.
 *   - Contacts. Every pair of a segment pixel and a node adjacent to it (one of the node's pixels lies among the pixel's eight
 *     neighbours) counts.
 *       - It adds 1 to contacts.
 *       - It adds 1 to ortho if a pixel of that node is among the pixel's four edge neighbours, else 1 to diag.
 *       - So a segment's length runs from node zone to node zone.
 *   - ends: the segment's pixels that are in END(A) of rsu_graph.h (isolated pixels included). Such a pixel is a node too, with id
 *     -(index + 1).
 *   - node_a / node_b: the smallest and largest id over all the segment's contacts and ends. Both are 0 when it has none, which means a
 *     closed ring.
 *
 * Reading a row.
 *   - A clean edge has contacts + ends == 2.
 *   - node_a == node_b > 0 is a loop through one node.
 *   - contacts + ends > 2 is the documented artefact "multi": two branches that still touch. node_a / node_b are then only the
 *     extremes.
 *   - length = ortho + sqrt(2) diag is formed by the caller, never on the device.
 *
 * Out of scope: ordered polylines along an edge (a sequential walk or a list ranking: a later step), and splitting "multi" segments.
 *
 * The method. A classify launch forms A, J and Z per pixel from a tile with a two-pixel halo in LDS and writes S_P, S_T, Z_P, Z_T as
 * four float32 planes into ws. rsu_components.h's labelling runs once over them as 4 N images (connectivity 8): its tile launch, M
 * merge launches, M = ceil(log2(max(ceil(H / 64), ceil(W / 64)))), and its flatten launch. Three launches order the segments: the roots
 * per block of 256 pixels are counted; one workgroup per image and side scans the block counts and writes `counts`; every root takes
 * its rank (ballot and popcount inside a block) and initialises its row. A measure launch over the pixels of the two S planes adds
 * every segment pixel's links, contacts and end flag to its segment's row with integer add / min / max atomics -- order-free, so every
 * result is a function of the inputs alone -- and writes seg_* and node_*. A finish launch, one workgroup per image and side, closes
 * the rows and adds to acc. The launch count,
 *     8 + M,
 * is fixed by N, H, W; no flag between workgroups, no grid-wide barrier, no float atomic.
 *
 * ws: rsu_segments_ws_bytes bytes, 8-byte aligned. It need not be cleared and holds nothing between calls. */
#define RSU_SEGMENTS_MAX_SIDE 1024
#define RSU_SEGMENTS_MAX_EDGES 65536
size_t rsu_segments_ws_bytes(int N, int H, int W, int max_edges);   /* 0 for refused sizes */

/* edges_pred, edges_true: int32 [N][max_edges][8], one row per segment of P / of T, in ascending label order:
 *        {label, pixels, ortho, diag, node_a, node_b, contacts, ends}.
 *      Only the first min(count, max_edges) rows are written. Rows at and past that are not touched.
 * counts: int32 [N][4], written: counts[n] = {segments of P, nodes of P, segments of T, nodes of T}. These are the true numbers, also
 *      when they exceed max_edges. An image without a counted pixel writes four zeros.
 * seg_pred, seg_true: int32 [N][H][W], may be NULL: the segment label at segment pixels, 0 elsewhere.
 * node_pred, node_true: int32 [N][H][W], may be NULL: the node id at zone pixels, -(index + 1) at segment pixels in END(A), 0 elsewhere.
 * acc: may be NULL; otherwise unsigned 64-bit [2][8], ACCUMULATED (the caller zeroes it):
 *        acc[side] += {rows stored, pixels, ortho, diag, dangling, free, rings, multi} over the stored rows (side 0 = P, 1 = T), with
 *          dangling: contacts == 1 && ends == 1,     free:  contacts == 0 && ends >= 1,
 *          rings:    contacts + ends == 0,           multi: contacts + ends > 2,
 *      updated with one 64-bit integer atomic per non-zero counter per workgroup.
 * labels64 may be NULL iff every *_true pointer is NULL: every pixel is then counted and T is empty. No overlap between any two buffers
 * is allowed.
 * RSU_EINVAL: N, H or W below 1; a side above RSU_SEGMENTS_MAX_SIDE; max_edges outside [1, RSU_SEGMENTS_MAX_EDGES]; a non-finite
 *      threshold; a NULL prob, ws, counts or edges_pred; edges_true NULL although labels64 is given; a *_true output given without
 *      labels64.
 * RSU_E2BIG: labels64 (N H W 8 bytes) or the entry's largest internal array (16 N H W bytes, the four int32 planes) reaches 0x7ffffff0.
 *      Without labels64 the second rule alone holds. At 1024 x 1024 the last admitted batch is 127 images, and 128 is refused.
 * An argument error is reported before the size. Nothing is written outside the outputs, acc[0 .. 15] and ws. */
/* align (rsu_line_segments): prob 4, labels64 8, edges_pred 4, edges_true 4, counts 4, seg_pred 4, seg_true 4, node_pred 4, node_true 4, acc 8,
 * ws 8. */
int rsu_line_segments(const float* prob, float threshold, const int64_t* labels64, int max_edges, int32_t* edges_pred, int32_t* edges_true,
                      int32_t* counts, int32_t* seg_pred, int32_t* seg_true, int32_t* node_pred, int32_t* node_true, unsigned long long* acc,
                      void* ws, int N, int H, int W, rsu_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RSU_SEGMENTS_H_ */
