/*
 * rsu_routes.h -- the twelfth public header of librsu_hip.so: the fifth step from a mask to a road network. It looks at the network as
 * a network: the node table of one side of rsu_segments.h, the length of the shortest path between every two nodes, and one direction
 * of a path-length score between two such graphs (APLS, the average path length similarity of Van Etten et al., SpaceNet, with the
 * graphs' own nodes as control points). It reads the outputs of one rsu_line_segments call, so the chain
 * thin -> prune -> segments -> routes never leaves the device.
 *
 * Same library, same conventions and memory contract as rsu.h (plain C, device pointers + sizes, `stream` a hipStream_t passed as
 * void*, asynchronous on that stream, 0 on success and a negative RSU_E* code otherwise, returned before anything is launched or
 * dereferenced; no allocation, no host synchronisation). tests/test_gpu_routes_fenced.py holds the launching entries of this header to
 * the memory contract; road_segmentation_unet_amd/_lib.py binds them through its table ROUTES_SIGNATURES.
 */
#ifndef RSU_ROUTES_H_
#define RSU_ROUTES_H_

#include "rsu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- network distances (new; the reference has none) ------------------------------------------------------------------------------- */
/* Inputs. They come from one rsu_line_segments call, for one side per call:
 *   node_map: int32 [N][H][W], node_pred or node_true: the node id at zone pixels, -(index + 1) at line ends, 0 elsewhere.
 *   edges:    int32 [N][max_edges][8], that side's rows {label, pixels, ortho, diag, node_a, node_b, contacts, ends}.
 *   counts:   int32 [N][4]. side 0 reads counts[n][0], side 1 reads counts[n][2].
 *   stored = min(count, max_edges) rows are read.
 *   images:   independent.
 *
 * Node table. A node is a non-zero id of node_map. Its ROOT pixel is p with node_map[p] == p + 1 (a zone's smallest pixel, by the
 * label's definition) or node_map[p] < 0 (a line end, whose id is -(p + 1)). Nodes are numbered in ascending root pixel index, which is
 * ascending |id|, unique per node. A row is {id, y, x, pixels}: an end's position is its pixel and its `pixels` is 1; a zone's position
 * is the rounded centroid, y = (2 sum(y) + pixels) / (2 pixels) in integer floor division and x likewise, over the pixels that hold its
 * id. The sums are taken with 32-bit integer atomics (order-free): sum(y) <= 1023 * 2^20 < 2^31; the quotient is formed in 64 bits. A
 * zone pixel finds its node's row by binary search on |id|.
 *
 * Edges. A stored row is an edge iff node_a != node_b: rings and loops through one node are skipped; a "multi" row joins its two
 * extremes. Its weight is w = min(70 ortho + 99 diag, RSU_ROUTES_INF), formed in 64 bits: 99 / 70 is a convergent of sqrt(2) with a
 * relative error of 5e-5, and a length in pixels is w / 70. The longest possible path, 99 * 2^20, is below RSU_ROUTES_INF, and the sum of
 * two entries never overflows int32. An edge row with a negative ortho or diag, or with a node that is not in the stored table, is
 * skipped and counted. Parallel edges keep the minimum (integer atomicMin).
 *
 * The method. Three launches compact the roots as rsu_segments.h compacts its segments: the roots per block of 256 pixels are counted;
 * one workgroup per image scans the block counts and writes info; every root takes its rank (ballot and popcount inside a block) and
 * writes its row. One launch fills the stored part of dist with RSU_ROUTES_INF and a zero diagonal, one adds the zone pixels to their
 * rows' sums, one closes the zone rows, one puts the edges into dist. Then a blocked Floyd-Warshall in integer min-plus,
 * min(a + b, RSU_ROUTES_INF), over 64 x 64 tiles (16 KB each) in LDS: each round r of the T = ceil(max_nodes / 64) rounds has three
 * phases: the diagonal tile (r, r), by one workgroup per image; the tiles of its row and of its column, each with the diagonal tile
 * beside it; the rest, C(I, J) = min(C, A(I, r) + B(r, J)), with A and B in LDS and C in registers (4 x 4 per thread). The first
 * diagonal tile has a launch of its own; every later one is swept by the workgroup of the third phase that finishes tile
 * (r + 1, r + 1) in the round before, so a round is two launches (three were 9 % slower per call). A workgroup writes
 * only its own tile and reads only tiles that an earlier launch finished. A launch returns at once for an image with 64 r >= stored
 * nodes, which it reads from info on the device, and so do tiles past the stored nodes: for a graph of at most 64 nodes one launch does
 * all the work. Loads and stores are masked at the stored count. The launch count,
 *     8 + 2 T,
 * is fixed by max_nodes; no float operation, no flag between workgroups, no grid-wide barrier. Min-plus has no matrix instruction: this
 * is VALU and LDS work.
 *
 * The kernels (gfx950, 256 threads each, no scratch; from the build's ISA):
 *     k_routes_count    6 VGPRs,    16 bytes of LDS, 8 waves per SIMD
 *     k_routes_scan    14 VGPRs,  1024 bytes of LDS, 8 waves per SIMD
 *     k_routes_place   10 VGPRs,    16 bytes of LDS, 8 waves per SIMD
 *     k_routes_fill     9 VGPRs,     0 bytes of LDS, 8 waves per SIMD
 *     k_routes_sums     9 VGPRs,     0 bytes of LDS, 8 waves per SIMD
 *     k_routes_close   24 VGPRs,     0 bytes of LDS, 8 waves per SIMD
 *     k_routes_edges   14 VGPRs,     8 bytes of LDS, 8 waves per SIMD
 *     k_routes_diag    56 VGPRs, 16384 bytes of LDS, 8 waves per SIMD
 *     k_routes_cross   74 VGPRs, 32768 bytes of LDS, 5 waves per SIMD
 *     k_routes_rest    82 VGPRs, 33792 bytes of LDS, 4 waves per SIMD
 *     k_routes_match   16 VGPRs,     0 bytes of LDS, 8 waves per SIMD
 *     k_routes_pairs   30 VGPRs,   16 bytes of LDS, 8 waves per SIMD
 *
 * ws: rsu_routes_ws_bytes bytes, 4-byte aligned: the root counts int32 [N][ceil(H W / 256)], then the zone sums int32 [N][max_nodes][3].
 * It need not be cleared and holds nothing between calls. */
#define RSU_ROUTES_MAX_SIDE 1024
#define RSU_ROUTES_MAX_NODES 1024
#define RSU_ROUTES_INF 0x3fffffff
#define RSU_ROUTES_Q 65536
size_t rsu_routes_ws_bytes(int N, int H, int W, int max_nodes);   /* 0 for refused sizes */

/* nodes: int32 [N][max_nodes][4] = {id, y, x, pixels}. Only the first min(nodes, max_nodes) rows are written. Rows at and past that are
 *      not touched.
 * dist: int32 [N][max_nodes][max_nodes]: dist[n][i][j] for i, j < stored nodes is the length of the shortest path from node i to node
 *      j, RSU_ROUTES_INF where there is none, and 0 on the diagonal. Every other element is not touched.
 * info: int32 [N][4] = {nodes (the true number), nodes stored, edges used, rows skipped for a node past max_nodes or an inconsistent
 *      row}, written, also for an empty image.
 * No overlap between any two buffers is allowed. Every index formed from node_map, edges and counts is range-checked before it addresses
 * memory: inconsistent inputs give unspecified values, never a write outside the outputs and ws.
 * RSU_EINVAL: N, H or W below 1; a side above RSU_ROUTES_MAX_SIDE; `side` not 0 or 1; max_edges outside [1, 65536]; max_nodes outside
 *      [1, RSU_ROUTES_MAX_NODES]; a NULL pointer.
 * RSU_E2BIG: node_map (4 N H W bytes) or dist (4 N max_nodes^2 bytes) reaches 0x7ffffff0. At 1024 x 1024, or at max_nodes 1024, the last
 *      admitted batch is 511 images, and 512 is refused.
 * An argument error is reported before the size. Nothing is written outside the outputs and ws. */
/* align (rsu_graph_routes): node_map 4, edges 4, counts 4, nodes 4, dist 4, info 4, ws 4. */
int rsu_graph_routes(const int32_t* node_map, const int32_t* edges, const int32_t* counts, int side, int max_edges, int max_nodes,
                     int32_t* nodes, int32_t* dist, int32_t* info, void* ws, int N, int H, int W, rsu_stream_t stream);

/* ---- one direction of the path-length score, from graph a to graph b ----------------------------------------------------------------- */
/* Both graphs are in the formats above and use the same max_nodes. The stored counts are read from info_a[n][1] and info_b[n][1].
 * match: int32 [N][max_nodes]: for every stored node i of a, the stored node j of b with the smallest (dy)^2 + (dx)^2; ties go to the
 *      smaller j. A node matches only if that distance is at most slack^2; otherwise the entry is -1. Rows at and past the stored count
 *      are not touched.
 * Pairs. Every pair i < k of a with 0 < d = dist_a[i][k] < RSU_ROUTES_INF is a pair. It contributes q in units of Q = RSU_ROUTES_Q:
 *      q = Q if either node is unmatched (counted in `unmatched`); q = Q if e = dist_b[match i][match k] is RSU_ROUTES_INF (counted in
 *      `broken`); q = min(Q, floor(Q |d - e| / d)) otherwise, formed in 64 bits.
 * acc: unsigned 64-bit [4], ACCUMULATED (the caller zeroes it): acc += {pairs, sum of q, unmatched, broken}. Partial sums stay inside a
 *      wave and a workgroup; one 64-bit integer atomic is issued per non-zero counter per workgroup: order-free, so the result is a
 *      function of the inputs. Two launches (match, pairs); no workspace.
 * The score of a direction is 1 - sum of q / (Q pairs). It is formed by the caller, never on the device.
 * Limits. The control points are the graph's own nodes (junction zones and line ends); points injected along edges, as the full APLS has
 * them, are a later step: the ordered paths of rsu_paths.h give the arc lengths that step needs. A path's length skips the interiors of
 * the node zones it crosses. Everything is per image.
 * RSU_EINVAL: N below 1; max_nodes outside [1, RSU_ROUTES_MAX_NODES]; slack outside [0, 1023]; a NULL pointer.
 * RSU_E2BIG: dist_a (4 N max_nodes^2 bytes) reaches 0x7ffffff0. An argument error is reported before the size. Nothing is written outside
 * match and acc[0 .. 3]. */
/* align (rsu_route_score): nodes_a 4, dist_a 4, info_a 4, nodes_b 4, dist_b 4, info_b 4, match 4, acc 8. */
int rsu_route_score(const int32_t* nodes_a, const int32_t* dist_a, const int32_t* info_a, const int32_t* nodes_b, const int32_t* dist_b,
                    const int32_t* info_b, int max_nodes, int slack, int32_t* match, unsigned long long* acc, int N, rsu_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* RSU_ROUTES_H_ */
