// Network distances and the path-length score (include/rsu_routes.h): the node table of one side of rsu_line_segments, the length of the
// shortest path between every two of its nodes by a blocked Floyd-Warshall in integer min-plus, and one direction of the score between
// two such graphs. Integer only; every result is a function of the inputs alone.
//
// A ROOT is a pixel p with node_map[p] == p + 1 (a zone's smallest pixel) or node_map[p] < 0 (a line end). Roots are compacted in
// ascending p as segments.hip compacts its segments; a node id is found again by binary search on |id|, which ascends with p.
//
// ws: the root counts int32 [N][ceil(H W / RT_BLOCK)] (exclusive offsets after the scan), then the zone sums int32 [N][max_nodes][3] =
// {sum y, sum x, pixels}: sum y <= 1023 * 2^20 < 2^31.
//
//   k_routes_count   the roots of every block of RT_BLOCK pixels.
//   k_routes_scan    one workgroup per image: the exclusive scan of the block counts; info = {nodes, nodes stored, 0, 0}.
//   k_routes_place   every root takes its rank (ballot and popcount inside a block), writes its row {id, y, x, 1} and clears its sums.
//   k_routes_fill    one workgroup per 64 x 64 tile of dist: RT_INF, 0 on the diagonal, for i, j < stored.
//   k_routes_sums    one thread per pixel: a zone pixel adds its position to its node's sums (integer atomics: order-free).
//   k_routes_close   one thread per stored node: a zone's rounded centroid and pixel count.
//   k_routes_edges   one thread per stored row: the weight of an edge row into dist[a][b] and dist[b][a] by atomicMin; the rows used and
//                    skipped are summed in LDS and added to info with one integer atomic per non-zero counter per workgroup.
//   k_routes_diag    round 0, the tile (0, 0): one workgroup per image; the tile in LDS, 64 steps. The diagonal tile of every later round is
//                    swept by the workgroup of k_routes_rest that finishes it in the round before (three launches per round were 9 %
//                    slower per call: profiles/r32/routes.txt).
//   k_routes_cross   round r, the tiles (r, J) and (I, r): the tile and the finished diagonal tile in LDS, 64 steps.
//   k_routes_rest    round r, every other tile: C(I, J) = min(C, A(I, r) + B(r, J)); A transposed (rows of RT_PAD words: the transposing
//                    stores are 4-way, not 64-way, on the banks, the 16-byte reads stay aligned) and B in LDS, C in registers. The
//                    workgroup of tile (r + 1, r + 1) then puts C into its B tile and runs round r + 1's diagonal sweep.
//   k_routes_match   one thread per stored node of a: the nearest stored node of b, ties to the smaller index.
//   k_routes_pairs   one workgroup per 64 x 64 tile of the upper triangle of dist_a: the pairs' contributions.
// In the 64-step kernels row k and column k of a tile do not change in step k (the diagonal is 0, or RT_INF past the stored nodes), and
// every step reads, meets a barrier, writes and meets a barrier. A workgroup writes only its own tile and reads only tiles that an earlier
// launch finished. No entry of dist exceeds RT_INF, so a + b stays inside int32 and min(c, a + b) needs no second clamp.
// No float operation, no flag between workgroups, no grid-wide barrier.
#include "routes.h"

#define RT_BLOCK 256   // threads of every launch
#define RT_TILE 64     // the Floyd-Warshall tile: RT_TILE x RT_TILE distances, 4 x 4 per thread
#define RT_PAD 68      // words per row of the transposed tile

namespace {

typedef unsigned long long u64;
constexpr int RT_WORDS = RT_TILE * RT_TILE;
static_assert(RT_BLOCK == 256 && RT_TILE == 64 && RT_WORDS == 16 * RT_BLOCK, "sixteen distances per thread");
static_assert(RT_PAD % 4 == 0 && RT_PAD >= RT_TILE, "the 16-byte reads of the transposed tile stay aligned");
static_assert((long)RT_INF * 2 < 0x7fffffffL, "the sum of two entries stays inside int32");

__device__ __forceinline__ int rt_clamp(int v, int hi) { return v < 0 ? 0 : (v < hi ? v : hi); }
__device__ __forceinline__ int rt_stored(const int32_t* info, unsigned n, int max_nodes) { return rt_clamp(info[(size_t)n * 4 + 1], max_nodes); }
__device__ __forceinline__ unsigned rt_abs(int v) { return v < 0 ? 0u - (unsigned)v : (unsigned)v; }
__device__ __forceinline__ bool rt_root(int v, unsigned i) { return v < 0 || (unsigned)v == i + 1; }

// the row of node `id` among the `stored` rows of one image's table, -1 if it has none
__device__ __forceinline__ int rt_find(const int32_t* __restrict__ table, int stored, int id) {
    const unsigned key = rt_abs(id);
    int lo = 0, hi = stored;   // the first row whose |id| is not below this one
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (rt_abs(table[(size_t)mid * 4]) < key)
            lo = mid + 1;
        else
            hi = mid;
    }
    return lo < stored && table[(size_t)lo * 4] == id ? lo : -1;
}

// a block's root count from the flags of its four waves; every thread gets it. `before`: the roots in the waves before this one
__device__ __forceinline__ int rt_block_roots(bool root, int* wsum, int& before, u64& ballot) {
    const int tid = threadIdx.x, wave = tid >> 6;
    ballot = __ballot(root);
    if ((tid & 63) == 0) wsum[wave] = __popcll(ballot);
    __syncthreads();
    int total = 0;
    before = 0;
#pragma unroll
    for (int w = 0; w < RT_BLOCK / 64; ++w) {
        const int v = wsum[w];
        if (w < wave) before += v;
        total += v;
    }
    return total;
}

// grid N * nblk
__global__ void __launch_bounds__(RT_BLOCK) k_routes_count(const int32_t* __restrict__ node_map, int* __restrict__ bc, unsigned HW, unsigned nblk) {
    __shared__ int wsum[RT_BLOCK / 64];
    const unsigned n = blockIdx.x / nblk, i = (blockIdx.x % nblk) * RT_BLOCK + threadIdx.x;
    const bool root = i < HW && rt_root(node_map[(size_t)n * HW + i], i);
    int before;
    u64 ballot;
    const int total = rt_block_roots(root, wsum, before, ballot);
    if (threadIdx.x == 0) bc[blockIdx.x] = total;
}

// grid N, block RT_BLOCK. bc [N][nblk]: the counts become exclusive offsets
__global__ void __launch_bounds__(RT_BLOCK) k_routes_scan(int* __restrict__ bc, int32_t* __restrict__ info, int max_nodes, unsigned nblk) {
    __shared__ int part[RT_BLOCK];
    const int tid = threadIdx.x;
    const unsigned n = blockIdx.x;
    int* s = bc + (size_t)n * nblk;
    const unsigned chunk = (nblk + RT_BLOCK - 1) / RT_BLOCK, lo = tid * chunk, hi = lo + chunk < nblk ? lo + chunk : nblk;
    int mine = 0;
    for (unsigned i = lo; i < hi; ++i) mine += s[i];
    part[tid] = mine;
    __syncthreads();
    for (int d = 1; d < RT_BLOCK; d <<= 1) {   // an inclusive scan of the 256 partial sums
        const int v = tid >= d ? part[tid - d] : 0;
        __syncthreads();
        part[tid] += v;
        __syncthreads();
    }
    int run = part[tid] - mine;
    for (unsigned i = lo; i < hi; ++i) {
        const int c = s[i];
        s[i] = run;
        run += c;
    }
    if (tid == 0) {
        const int total = part[RT_BLOCK - 1];
        info[(size_t)n * 4] = total;
        info[(size_t)n * 4 + 1] = total < max_nodes ? total : max_nodes;
        info[(size_t)n * 4 + 2] = 0;
        info[(size_t)n * 4 + 3] = 0;
    }
}

// grid N * nblk. nodes [N][max_nodes][4], sums [N][max_nodes][3]
__global__ void __launch_bounds__(RT_BLOCK) k_routes_place(const int32_t* __restrict__ node_map, const int* __restrict__ bc, int32_t* __restrict__ nodes,
                                                           int* __restrict__ sums, int max_nodes, int W, unsigned HW, unsigned nblk) {
    __shared__ int wsum[RT_BLOCK / 64];
    const unsigned n = blockIdx.x / nblk, i = (blockIdx.x % nblk) * RT_BLOCK + threadIdx.x;
    const int v = i < HW ? node_map[(size_t)n * HW + i] : 0;
    const bool root = i < HW && rt_root(v, i);
    int before;
    u64 ballot;
    rt_block_roots(root, wsum, before, ballot);
    if (!root) return;
    const int r = bc[blockIdx.x] + before + __popcll(ballot & ((1ull << (threadIdx.x & 63)) - 1ull));
    if (r < 0 || r >= max_nodes) return;
    const size_t at = (size_t)n * max_nodes + r;
    int32_t* row = nodes + at * 4;
    row[0] = v;
    row[1] = (int)(i / (unsigned)W);
    row[2] = (int)(i % (unsigned)W);
    row[3] = 1;
    sums[at * 3] = sums[at * 3 + 1] = sums[at * 3 + 2] = 0;
}

// grid N * T * T
__global__ void __launch_bounds__(RT_BLOCK) k_routes_fill(int32_t* __restrict__ dist, const int32_t* __restrict__ info, int max_nodes, unsigned T) {
    const unsigned n = blockIdx.x / (T * T), t = blockIdx.x % (T * T);
    const int i0 = (int)(t / T) * RT_TILE, j0 = (int)(t % T) * RT_TILE;
    const int stored = rt_stored(info, n, max_nodes);
    if (i0 >= stored || j0 >= stored) return;
    int32_t* d = dist + (size_t)n * max_nodes * max_nodes;
#pragma unroll
    for (int s = 0; s < RT_WORDS / RT_BLOCK; ++s) {
        const int idx = (int)threadIdx.x + s * RT_BLOCK, i = i0 + (idx >> 6), j = j0 + (idx & 63);
        if (i < stored && j < stored) d[(size_t)i * max_nodes + j] = i == j ? 0 : RT_INF;
    }
}

// grid N * nblk
__global__ void __launch_bounds__(RT_BLOCK) k_routes_sums(const int32_t* __restrict__ node_map, const int32_t* __restrict__ nodes,
                                                          const int32_t* __restrict__ info, int* __restrict__ sums, int max_nodes, int W, unsigned HW,
                                                          unsigned nblk) {
    const unsigned n = blockIdx.x / nblk, i = (blockIdx.x % nblk) * RT_BLOCK + threadIdx.x;
    if (i >= HW) return;
    const int v = node_map[(size_t)n * HW + i];
    if (v <= 0) return;
    const int r = rt_find(nodes + (size_t)n * max_nodes * 4, rt_stored(info, n, max_nodes), v);
    if (r < 0) return;
    int* s = sums + ((size_t)n * max_nodes + r) * 3;
    atomicAdd(&s[0], (int)(i / (unsigned)W));
    atomicAdd(&s[1], (int)(i % (unsigned)W));
    atomicAdd(&s[2], 1);
}

// grid N * ceil(max_nodes / RT_BLOCK)
__global__ void __launch_bounds__(RT_BLOCK) k_routes_close(int32_t* __restrict__ nodes, const int32_t* __restrict__ info, const int* __restrict__ sums,
                                                           int max_nodes, unsigned per) {
    const unsigned n = blockIdx.x / per;
    const int r = (int)((blockIdx.x % per) * RT_BLOCK + threadIdx.x);
    if (r >= rt_stored(info, n, max_nodes)) return;
    const size_t at = (size_t)n * max_nodes + r;
    int32_t* row = nodes + at * 4;
    const long long pixels = sums[at * 3 + 2];
    if (row[0] <= 0 || pixels <= 0) return;
    row[1] = (int)((2ll * sums[at * 3] + pixels) / (2ll * pixels));
    row[2] = (int)((2ll * sums[at * 3 + 1] + pixels) / (2ll * pixels));
    row[3] = (int)pixels;
}

// grid N * ceil(max_edges / RT_BLOCK)
__global__ void __launch_bounds__(RT_BLOCK) k_routes_edges(const int32_t* __restrict__ edges, const int32_t* __restrict__ counts, int side, int max_edges,
                                                           const int32_t* __restrict__ nodes, int32_t* __restrict__ info, int32_t* __restrict__ dist,
                                                           int max_nodes, unsigned per) {
    __shared__ int tally[2];   // rows used, rows skipped
    const unsigned n = blockIdx.x / per;
    const int e = (int)((blockIdx.x % per) * RT_BLOCK + threadIdx.x);
    if (threadIdx.x < 2) tally[threadIdx.x] = 0;
    __syncthreads();
    const int rows = rt_clamp(counts[(size_t)n * 4 + 2 * side], max_edges);
    int used = 0, skipped = 0;
    if (e < rows) {
        const int32_t* row = edges + ((size_t)n * max_edges + e) * 8;
        const int ortho = row[2], diag = row[3], a = row[4], b = row[5];
        if (a != b) {   // (a ring or a loop through one node is no edge)
            const int stored = rt_stored(info, n, max_nodes);
            const int32_t* table = nodes + (size_t)n * max_nodes * 4;
            const int ia = rt_find(table, stored, a), ib = rt_find(table, stored, b);
            if (ortho < 0 || diag < 0 || ia < 0 || ib < 0) {
                skipped = 1;
            } else {
                const long long w64 = 70ll * ortho + 99ll * diag;
                const int w = w64 < RT_INF ? (int)w64 : RT_INF;
                int32_t* d = dist + (size_t)n * max_nodes * max_nodes;
                atomicMin(&d[(size_t)ia * max_nodes + ib], w);
                atomicMin(&d[(size_t)ib * max_nodes + ia], w);
                used = 1;
            }
        }
    }
    const int u = __popcll(__ballot(used)), s = __popcll(__ballot(skipped));
    if ((threadIdx.x & 63) == 0) {
        if (u) atomicAdd(&tally[0], u);
        if (s) atomicAdd(&tally[1], s);
    }
    __syncthreads();
    if (threadIdx.x < 2 && tally[threadIdx.x]) atomicAdd(&info[(size_t)n * 4 + 2 + threadIdx.x], tally[threadIdx.x]);
}

// one tile of dist into LDS, row-major; RT_INF at and past the stored nodes
__device__ __forceinline__ void rt_load(int* __restrict__ t, const int32_t* __restrict__ d, int max_nodes, int stored, int i0, int j0) {
#pragma unroll
    for (int s = 0; s < RT_WORDS / RT_BLOCK; ++s) {
        const int idx = (int)threadIdx.x + s * RT_BLOCK, i = i0 + (idx >> 6), j = j0 + (idx & 63);
        t[idx] = i < stored && j < stored ? d[(size_t)i * max_nodes + j] : RT_INF;
    }
}
__device__ __forceinline__ void rt_store(const int* __restrict__ t, int32_t* __restrict__ d, int max_nodes, int stored, int i0, int j0) {
#pragma unroll
    for (int s = 0; s < RT_WORDS / RT_BLOCK; ++s) {
        const int idx = (int)threadIdx.x + s * RT_BLOCK, i = i0 + (idx >> 6), j = j0 + (idx & 63);
        if (i < stored && j < stored) d[(size_t)i * max_nodes + j] = t[idx];
    }
}

// C[i][j] = min(C[i][j], A[i][k] + B[k][j]) for k = 0 .. 63 in order, all three row-major tiles in LDS, where C is A, B or both. Thread
// (ty, tx) owns rows 4 ty .. and columns 4 tx .. of C. The caller has met a barrier behind the loads; the last step ends with one.
__device__ __forceinline__ void rt_sweep(const int* A, const int* B, int* C) {
    const int ty = (int)threadIdx.x >> 4, tx = (int)threadIdx.x & 15;
    int4 c[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) c[q] = *(const int4*)&C[(4 * ty + q) * RT_TILE + 4 * tx];
    for (int k = 0; k < RT_TILE; ++k) {
        int a[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) a[q] = A[(4 * ty + q) * RT_TILE + k];
        const int4 b = *(const int4*)&B[k * RT_TILE + 4 * tx];
        __syncthreads();   // every read of this step before any write of it
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            c[q].x = min(c[q].x, a[q] + b.x);
            c[q].y = min(c[q].y, a[q] + b.y);
            c[q].z = min(c[q].z, a[q] + b.z);
            c[q].w = min(c[q].w, a[q] + b.w);
            *(int4*)&C[(4 * ty + q) * RT_TILE + 4 * tx] = c[q];
        }
        __syncthreads();
    }
}

// grid N
__global__ void __launch_bounds__(RT_BLOCK) k_routes_diag(int32_t* __restrict__ dist, const int32_t* __restrict__ info, int max_nodes, int r) {
    __shared__ __attribute__((aligned(16))) int tile[RT_WORDS];
    const unsigned n = blockIdx.x;
    const int stored = rt_stored(info, n, max_nodes), k0 = r * RT_TILE;
    if (k0 >= stored) return;   // (the same for the whole workgroup)
    int32_t* d = dist + (size_t)n * max_nodes * max_nodes;
    rt_load(tile, d, max_nodes, stored, k0, k0);
    __syncthreads();
    rt_sweep(tile, tile, tile);
    rt_store(tile, d, max_nodes, stored, k0, k0);
}

// grid N * 2 * T: (n, which, t): which 0 = the tile (r, t) of the round's row, 1 = the tile (t, r) of its column
__global__ void __launch_bounds__(RT_BLOCK) k_routes_cross(int32_t* __restrict__ dist, const int32_t* __restrict__ info, int max_nodes, int r, unsigned T) {
    __shared__ __attribute__((aligned(16))) int pivot[RT_WORDS];
    __shared__ __attribute__((aligned(16))) int tile[RT_WORDS];
    const unsigned n = blockIdx.x / (2 * T), which = (blockIdx.x / T) & 1u;
    const int t = (int)(blockIdx.x % T);
    const int stored = rt_stored(info, n, max_nodes), k0 = r * RT_TILE, t0 = t * RT_TILE;
    if (k0 >= stored || t == r || t0 >= stored) return;
    int32_t* d = dist + (size_t)n * max_nodes * max_nodes;
    const int i0 = which ? t0 : k0, j0 = which ? k0 : t0;
    rt_load(pivot, d, max_nodes, stored, k0, k0);
    rt_load(tile, d, max_nodes, stored, i0, j0);
    __syncthreads();
    if (which)
        rt_sweep(tile, pivot, tile);
    else
        rt_sweep(pivot, tile, tile);
    rt_store(tile, d, max_nodes, stored, i0, j0);
}

// grid N * T * T
__global__ void __launch_bounds__(RT_BLOCK) k_routes_rest(int32_t* __restrict__ dist, const int32_t* __restrict__ info, int max_nodes, int r, unsigned T) {
    __shared__ __attribute__((aligned(16))) int At[RT_TILE * RT_PAD];   // A(I, r), transposed: At[k][i]
    __shared__ __attribute__((aligned(16))) int B[RT_WORDS];            // B(r, J)
    const unsigned n = blockIdx.x / (T * T), t = blockIdx.x % (T * T);
    const int I = (int)(t / T), J = (int)(t % T);
    const int stored = rt_stored(info, n, max_nodes), k0 = r * RT_TILE, i0 = I * RT_TILE, j0 = J * RT_TILE;
    if (k0 >= stored || I == r || J == r || i0 >= stored || j0 >= stored) return;
    int32_t* d = dist + (size_t)n * max_nodes * max_nodes;
#pragma unroll
    for (int s = 0; s < RT_WORDS / RT_BLOCK; ++s) {
        const int idx = (int)threadIdx.x + s * RT_BLOCK, i = idx >> 6, k = idx & 63;
        At[k * RT_PAD + i] = i0 + i < stored && k0 + k < stored ? d[(size_t)(i0 + i) * max_nodes + k0 + k] : RT_INF;
    }
    rt_load(B, d, max_nodes, stored, k0, j0);
    const int ty = (int)threadIdx.x >> 4, tx = (int)threadIdx.x & 15;
    int c[4][4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int i = i0 + 4 * ty + q, j = j0 + 4 * tx + p;
            c[q][p] = i < stored && j < stored ? d[(size_t)i * max_nodes + j] : RT_INF;
        }
    __syncthreads();
#pragma unroll 8
    for (int k = 0; k < RT_TILE; ++k) {
        const int4 a4 = *(const int4*)&At[k * RT_PAD + 4 * ty];
        const int4 b4 = *(const int4*)&B[k * RT_TILE + 4 * tx];
        const int a[4] = {a4.x, a4.y, a4.z, a4.w}, b[4] = {b4.x, b4.y, b4.z, b4.w};
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int p = 0; p < 4; ++p) c[q][p] = min(c[q][p], a[q] + b[p]);
    }
    if (I == r + 1 && J == r + 1) {   // the next round's diagonal tile: its sweep follows at once, and that round has no launch for it
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q) *(int4*)&B[(4 * ty + q) * RT_TILE + 4 * tx] = make_int4(c[q][0], c[q][1], c[q][2], c[q][3]);
        __syncthreads();
        rt_sweep(B, B, B);
        rt_store(B, d, max_nodes, stored, i0, j0);
        return;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int i = i0 + 4 * ty + q, j = j0 + 4 * tx + p;
            if (i < stored && j < stored) d[(size_t)i * max_nodes + j] = c[q][p];
        }
}

// grid N * ceil(max_nodes / RT_BLOCK)
__global__ void __launch_bounds__(RT_BLOCK) k_routes_match(const int32_t* __restrict__ nodes_a, const int32_t* __restrict__ info_a,
                                                           const int32_t* __restrict__ nodes_b, const int32_t* __restrict__ info_b, int max_nodes,
                                                           int slack, int32_t* __restrict__ match, unsigned per) {
    const unsigned n = blockIdx.x / per;
    const int i = (int)((blockIdx.x % per) * RT_BLOCK + threadIdx.x);
    if (i >= rt_stored(info_a, n, max_nodes)) return;
    const int sb = rt_stored(info_b, n, max_nodes);
    const int32_t* me = nodes_a + ((size_t)n * max_nodes + i) * 4;
    const int32_t* other = nodes_b + (size_t)n * max_nodes * 4;
    const long long y = me[1], x = me[2];
    long long best = (long long)slack * slack + 1;   // (only a distance of at most slack^2 matches)
    int at = -1;
    for (int j = 0; j < sb; ++j) {   // (the same j in every lane: the loads are broadcasts)
        const long long dy = y - other[(size_t)j * 4 + 1], dx = x - other[(size_t)j * 4 + 2], d2 = dy * dy + dx * dx;
        if (d2 < best) {   // (strictly: a tie stays with the smaller j)
            best = d2;
            at = j;
        }
    }
    match[(size_t)n * max_nodes + i] = at;
}

// grid N * T * T: the tile (I, K) of dist_a's upper triangle
__global__ void __launch_bounds__(RT_BLOCK) k_routes_pairs(const int32_t* __restrict__ dist_a, const int32_t* __restrict__ info_a,
                                                           const int32_t* __restrict__ dist_b, const int32_t* __restrict__ info_b,
                                                           const int32_t* __restrict__ match, int max_nodes, u64* __restrict__ acc, unsigned T) {
    __shared__ unsigned sums[4];   // pairs, q, unmatched, broken: at most 4096 pairs of at most 2^16 each
    const unsigned n = blockIdx.x / (T * T), t = blockIdx.x % (T * T);
    const int I = (int)(t / T), K = (int)(t % T);
    const int sa = rt_stored(info_a, n, max_nodes), sb = rt_stored(info_b, n, max_nodes);
    if (I > K || K * RT_TILE >= sa) return;   // (the same for the whole workgroup)
    if (threadIdx.x < 4) sums[threadIdx.x] = 0;
    __syncthreads();
    const size_t img = (size_t)n * max_nodes * max_nodes;
    const int32_t* m = match + (size_t)n * max_nodes;
    unsigned v[4] = {0, 0, 0, 0};
    for (int s = 0; s < RT_WORDS / RT_BLOCK; ++s) {
        const int idx = (int)threadIdx.x + s * RT_BLOCK, i = I * RT_TILE + (idx >> 6), k = K * RT_TILE + (idx & 63);
        if (i >= k || k >= sa) continue;
        const int d = dist_a[img + (size_t)i * max_nodes + k];
        if (d <= 0 || d >= RT_INF) continue;
        const int mi = m[i], mk = m[k];
        unsigned q = RT_Q;
        if (mi < 0 || mi >= sb || mk < 0 || mk >= sb) {
            v[2] += 1;
        } else {
            const int e = dist_b[img + (size_t)mi * max_nodes + mk];
            if (e >= RT_INF || e < 0) {
                v[3] += 1;
            } else {
                const u64 diff = (u64)(d > e ? d - e : e - d);
                if (diff < (u64)d) q = (unsigned)(diff * RT_Q / (u64)d);
            }
        }
        v[0] += 1;
        v[1] += q;
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {   // summed inside the wave first
        unsigned x = v[c];
#pragma unroll
        for (int d = 32; d; d >>= 1) x += __shfl_xor(x, d);
        if ((threadIdx.x & 63) == 0 && x) atomicAdd(&sums[c], x);
    }
    __syncthreads();
    if (threadIdx.x < 4 && sums[threadIdx.x]) atomicAdd(&acc[threadIdx.x], (u64)sums[threadIdx.x]);
}

inline unsigned rt_nblk(int H, int W) { return ((unsigned)(H * W) + RT_BLOCK - 1) / RT_BLOCK; }

}  // namespace

int rt_rounds(int max_nodes) { return (max_nodes + RT_TILE - 1) / RT_TILE; }

size_t rt_ws_bytes(int N, int H, int W, int max_nodes) { return ((size_t)N * rt_nblk(H, W) + (size_t)N * max_nodes * 3) * sizeof(int); }

int rt_launches(int max_nodes) { return 8 + 2 * rt_rounds(max_nodes); }

hipError_t rt_graph_routes(const int32_t* node_map, const int32_t* edges, const int32_t* counts, int side, int max_edges, int max_nodes,
                           int32_t* nodes, int32_t* dist, int32_t* info, void* ws, int N, int H, int W, hipStream_t st) {
    const unsigned HW = (unsigned)(H * W), nblk = rt_nblk(H, W), T = (unsigned)rt_rounds(max_nodes);
    const unsigned per_nodes = ((unsigned)max_nodes + RT_BLOCK - 1) / RT_BLOCK, per_edges = ((unsigned)max_edges + RT_BLOCK - 1) / RT_BLOCK;
    int* bc = (int*)ws;
    int* sums = bc + (size_t)N * nblk;
    const dim3 block(RT_BLOCK), pixels((unsigned)N * nblk), tiles((unsigned)N * T * T);
    hipLaunchKernelGGL(k_routes_count, pixels, block, 0, st, node_map, bc, HW, nblk);
    hipLaunchKernelGGL(k_routes_scan, dim3((unsigned)N), block, 0, st, bc, info, max_nodes, nblk);
    hipLaunchKernelGGL(k_routes_place, pixels, block, 0, st, node_map, (const int*)bc, nodes, sums, max_nodes, W, HW, nblk);
    hipLaunchKernelGGL(k_routes_fill, tiles, block, 0, st, dist, (const int32_t*)info, max_nodes, T);
    hipLaunchKernelGGL(k_routes_sums, pixels, block, 0, st, node_map, (const int32_t*)nodes, (const int32_t*)info, sums, max_nodes, W, HW, nblk);
    hipLaunchKernelGGL(k_routes_close, dim3((unsigned)N * per_nodes), block, 0, st, nodes, (const int32_t*)info, (const int*)sums, max_nodes, per_nodes);
    hipLaunchKernelGGL(k_routes_edges, dim3((unsigned)N * per_edges), block, 0, st, edges, counts, side, max_edges, (const int32_t*)nodes, info, dist,
                       max_nodes, per_edges);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    for (int r = 0; r < (int)T; ++r) {
        if (r == 0) hipLaunchKernelGGL(k_routes_diag, dim3((unsigned)N), block, 0, st, dist, (const int32_t*)info, max_nodes, r);
        hipLaunchKernelGGL(k_routes_cross, dim3((unsigned)N * 2 * T), block, 0, st, dist, (const int32_t*)info, max_nodes, r, T);
        hipLaunchKernelGGL(k_routes_rest, tiles, block, 0, st, dist, (const int32_t*)info, max_nodes, r, T);
    }
    return hipGetLastError();
}

hipError_t rt_route_score(const int32_t* nodes_a, const int32_t* dist_a, const int32_t* info_a, const int32_t* nodes_b, const int32_t* dist_b,
                          const int32_t* info_b, int max_nodes, int slack, int32_t* match, unsigned long long* acc, int N, hipStream_t st) {
    const unsigned T = (unsigned)rt_rounds(max_nodes), per = ((unsigned)max_nodes + RT_BLOCK - 1) / RT_BLOCK;
    const dim3 block(RT_BLOCK);
    hipLaunchKernelGGL(k_routes_match, dim3((unsigned)N * per), block, 0, st, nodes_a, info_a, nodes_b, info_b, max_nodes, slack, match, per);
    hipLaunchKernelGGL(k_routes_pairs, dim3((unsigned)N * T * T), block, 0, st, dist_a, info_a, dist_b, info_b, (const int32_t*)match, max_nodes, acc, T);
    return hipGetLastError();
}
