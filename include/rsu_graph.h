/*
 * rsu_graph.h -- the ninth public header of librsu_hip.so: the second step from a mask to a road graph. It prunes the short branches
 * (spurs) off a centre-line on the device and marks where the pruned lines end and where they meet: Gonzalez & Woods' morphological
 * pruning of a predicted and of a truth mask, then the ends, isolated pixels and junction pixels of the result. It reads and writes the
 * formats of rsu_thin.h, rsu_distance.h and rsu_components.h, so the chain thin -> prune -> nodes -> distances / components never
 * leaves the device.
 *
 * Same library, same conventions and memory contract as rsu.h and rsu_thin.h (plain C, device pointers + sizes, `stream` a hipStream_t
 * passed as void*, asynchronous on that stream, 0 on success and a negative RSU_E* code otherwise, returned before anything is
 * launched or dereferenced; no allocation, no host synchronisation). tests/test_gpu_graph_fenced.py holds the launching entry of this
 * header to the memory contract; road_segmentation_unet_amd/_lib.py binds it through its table SIGNATURES_GRAPH.
 */
#ifndef RSU_GRAPH_H_
#define RSU_GRAPH_H_

#include "rsu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- centre-line pruning and nodes (new; the reference has none) ------------------------------------------------------------------ */
/* prob is float32 [N][H][W], labels64 int64 [N][H][W]. The masks are rsu_thin.h's, word for word:
 *   images:   independent. Everything outside an image is background.
 *   counted:  a pixel is COUNTED iff its labels64 value is 0 or 1 (all 64 bits tested).
 *   P:        {counted and prob >= threshold}: one float32 comparison, the only float operation of this header. NaN is outside P,
 *             p == threshold is inside.
 *   T:        {labels64 == 1}. Ignored pixels are background on both sides.
 * So the entry takes the two outputs of rsu_mask_thin as they are (skel_pred at threshold 0.5 as prob, skel_true as labels64); it is
 * defined on any mask all the same.
 *
 *   rule:     let A be either mask, p2 .. p9 the neighbours of a pixel clockwise from north (p2 = N, p3 = NE, p4 = E, p5 = SE, p6 = S,
 *             p7 = SW, p8 = W, p9 = NW; cyclic: p9 is followed by p2), and
 *               n8 = the number of set neighbours,
 *               X  = the number of i with p_i == 0 and p_{i+1} == 1 (the crossing number).
 *             END(A) = A and X <= 1 and n8 <= 3: an isolated pixel, or a pixel whose neighbours form ONE run of at most three. (Guo &
 *             Hall's N == 1 is not enough: a one-pixel bump on a straight line has two neighbours; it would never go and the line
 *             pixel under it would stay a false junction.)
 *   pruning:  with L = min_branch,
 *               1. X1 = A; then L times X1 &= ~END(X1), all pixels at once from the state before;
 *               2. E = END(X1); then L times E = A and dilate8(E), the 3 x 3 dilation (E itself included) inside A;
 *               3. B = X1 | E.
 *             (Gonzalez & Woods, Digital Image Processing, "pruning".) A branch of at most L pixels is removed, a longer one is kept
 *             whole; a free curve of at most 2 L pixels vanishes, one of 2 L + 1 or more returns whole; a closed loop is untouched.
 *             L == 0 gives B = A and launches no prune step.
 *             KNOWN ARTEFACT: step 2 grows back everything of A within L pixels (geodesic, 8-connected) of a surviving end, so a
 *             spur that sits within L pixels of a true line end returns with that end.
 *   nodes:    of B: an END is a pixel of END(B) with n8 >= 1, an ISOLATED pixel one with n8 == 0, a JUNCTION PIXEL a pixel of B with
 *             X >= 3. Adjacent junction pixels are one junction: count them with rsu_components_pair_count at connectivity 8.
 *             A line that leaves the image ends there and is an END, on both sides alike.
 *   limits:   N, H, W >= 1, H, W <= RSU_GRAPH_MAX_SIDE, 0 <= min_branch <= RSU_GRAPH_MAX_BRANCH, threshold finite: RSU_EINVAL
 *             otherwise, for a NULL prob or ws, without any output and for a *_true output without labels64. RSU_E2BIG when prob,
 *             labels64 or an output reaches 0x7ffffff0 bytes (with labels64: N * H * W * 8, else N * H * W * 4).
 *
 * The method: both masks live in ws as bit rows, 64 - 2 R pixels to a 64-bit word (R = 16 rounds per launch: csrc/graph.h). An init
 * launch builds them from prob, threshold and labels64. Every step launch carries a tile -- one word wide, a workgroup's threads high --
 * through up to R rounds in registers and LDS: a thread holds one row of the tile as ONE 64-bit word, the word's own pixels with R
 * pixels of its neighbours to either side, and evaluates the rule bit-sliced, 64 pixels per operation (n8 and X as adder networks over
 * the eight neighbour words). A round looks one pixel out, so after R of them the core of the tile is exact and the halo is dropped.
 * ceil(L / R) delete launches are followed by ceil((L + 1) / R) regrow launches (the first of them forms END(X1), which costs it one
 * round). A step launch adds what it changed, per image and mask, to a counter of its own in ws (integer atomics, one per workgroup);
 * the NEXT launch reads it and returns at once where it is 0 -- a delete phase at its fixed point has no END pixel, so its regrow phase
 * returns too. A final launch forms B, classifies it and writes the outputs and counts. The launch count,
 *     2                                       for L == 0,
 *     2 + ceil(L / R) + ceil((L + 1) / R)     otherwise,
 * is fixed by the arguments; no flag between workgroups, no grid-wide barrier, no float atomic: every result is a function of the
 * inputs alone.
 *
 * ws: rsu_graph_ws_bytes bytes, 8-byte aligned. It need not be cleared and holds nothing between calls. */
#define RSU_GRAPH_MAX_SIDE 1024
#define RSU_GRAPH_MAX_BRANCH 64
size_t rsu_graph_ws_bytes(int N, int H, int W, int min_branch);      /* 0 for refused sizes */

/* out_pred:  float32 [N][H][W], 1.0 on the pruned B of P and 0.0 elsewhere.
 * out_true:  int64 [N][H][W], 1 on the pruned B of T and 0 on every other counted pixel; an ignored pixel keeps its labels64 value.
 * junc_pred, junc_true: the junction pixels of the two B, in the same two formats.
 * Each output may be NULL, not all four. labels64 may be NULL iff out_true and junc_true are: every pixel is then counted and T is empty.
 * out_pred == prob and out_true == labels64 are allowed (the masks are read by the init launch, and the final launch reads each label
 * before the same thread writes it); no other overlap is.
 * acc: may be NULL; otherwise unsigned 64-bit [8], ACCUMULATED (the caller zeroes it):
 *        acc[0 .. 3] += {|B|, ends, isolated pixels, junction pixels} of P,   acc[4 .. 7] += the same of T,
 *      with one integer atomic add per non-zero counter per workgroup. An image without a counted pixel adds exactly nothing.
 * Nothing is written outside the four outputs, acc[0 .. 7] and ws. */
/* align (rsu_skeleton_graph): prob 4, labels64 8, out_pred 4, out_true 8, junc_pred 4, junc_true 8, acc 8, ws 8. */
int rsu_skeleton_graph(const float* prob, float threshold, const int64_t* labels64, int min_branch, float* out_pred, int64_t* out_true,
                       float* junc_pred, int64_t* junc_true, unsigned long long* acc, void* ws, int N, int H, int W, rsu_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RSU_GRAPH_H_ */
