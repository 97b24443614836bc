#include "components.h"

// Connected components of a binary mask per image (include/rsu_components.h). A component's label is 1 + the smallest row-major index of
// its pixels, so a union-find that always links the larger root to the smaller one ends with the label in the root, whatever the order.
// The parent arrays hold `parent index + 1`, 0 at a background pixel; a root holds its own index + 1. Parents only decrease: every loop
// below (find, the union's retry) ends by that invariant alone and waits for nobody.
//   k_cc_tile     one workgroup per 64 x 64 tile: the mask (one ballot per row), every pixel's parent = the start of its horizontal run,
//                 the unions with the row above in LDS (atomicMin on the larger root), then every pixel's parent written as the image
//                 index of its tile root (row-major order in a tile agrees with the image's), the tile's area and edge flag of every
//                 tile root (one LDS add per run) and a zero total per pixel
//   k_cc_merge    level m = 1 .. cc_levels: one workgroup per 2^m x 2^m group of tiles unites the pixel pairs across the group's two new
//                 inner borders. A set a workgroup touches lies inside its group, so no two workgroups of a launch share a set: the
//                 per-XCD L2s need not agree inside a launch. The atomics are global atomicMin among the threads of ONE workgroup; find
//                 reads parents with relaxed agent-scope loads (no L1 line stands in for another wave's link)
//   k_cc_flatten  every pixel walks to its root (nothing writes the parents here) and writes its label; a tile root adds its tile's area
//                 to the root's total and ORs its edge flag in: one atomic pair per tile-level component, integer add / or
//   k_cc_gather_* area / edge per pixel, or the filter's decision and its counts (ballots, then one 64-bit integer add per workgroup)
// The only float operation is `p >= threshold`. The launch count is a function of the sizes and the arguments.
constexpr int CC_THREADS = 256;
constexpr int CC_ROWS = CC_TILE / (CC_THREADS / 64);   // rows of a tile per wave
constexpr int CC_PIX = CC_TILE * CC_TILE;
static_assert(CC_TILE == 64 && CC_THREADS == 256, "a tile row is one 64-lane ballot, four waves share the 64 rows");

enum { CC_FG = 0, CC_INV = 1, CC_HOLES = 2, CC_PRED = 3, CC_TRUTH = 4 };
// what a labelling labels. A launch covers `planes` = N or 2 N masks: plane q is image q % N in mode `mode + q / N` (the pair count labels
// the prediction and the truth of every image in one sequence of launches)
struct CcSrc {
    const float* prob;
    const int64_t* labels64;   // CC_PRED, CC_TRUTH
    const int* lab1;           // CC_HOLES: the labels and totals of the filter's first labelling, nullptr when it was skipped
    const int* tot1;
    float thr;
    int min_area;
    int mode;
};
// g = n * HW + the pixel's index, base = n * HW
__device__ __forceinline__ bool cc_foreground(const CcSrc& s, int mode, size_t g, size_t base) {
    switch (mode) {
        case CC_FG: return s.prob[g] >= s.thr;
        case CC_INV: return !(s.prob[g] >= s.thr);
        case CC_HOLES: {
            if (!(s.prob[g] >= s.thr)) return true;
            if (!s.lab1) return false;
            const int l = s.lab1[g];   // (a foreground pixel of the first labelling: l >= 1)
            return (s.tot1[base + (size_t)(l - 1)] & CC_AREA) < s.min_area;
        }
        case CC_PRED: {
            const int64_t lab = s.labels64[g];
            return (lab == 0 || lab == 1) && s.prob[g] >= s.thr;
        }
        default: return s.labels64[g] == 1;
    }
}

// ---- union-find on the tile's parents in LDS (plain indices; -1 = background, never reached) ----
__device__ __forceinline__ int cc_lds_find(int* p, int i) {
    for (;;) {
        const int v = __hip_atomic_load(&p[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (v == i) return i;
        i = v;   // (v < i)
    }
}
__device__ __forceinline__ void cc_lds_union(int* p, int a, int b) {
    for (;;) {
        a = cc_lds_find(p, a);
        b = cc_lds_find(p, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(&p[a], b);
        if (old == a) return;   // a was a root and now hangs under b
        a = old;                // a had a parent `old` < a already (and hangs under min(old, b) now): unite that one with b
    }
}
// ---- and on an image's parents in global memory (index + 1), among the threads of one workgroup ----
__device__ __forceinline__ int cc_find(int* p, int i) {
    for (;;) {
        const int v = __hip_atomic_load(&p[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - 1;
        if (v == i) return i;
        i = v;
    }
}
__device__ __forceinline__ void cc_union(int* p, int a, int b) {
    for (;;) {
        a = cc_find(p, a);
        b = cc_find(p, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = atomicMin(&p[a], b + 1) - 1;
        if (old == a) return;
        a = old;
    }
}

// grid: planes * tiles_y * tiles_x workgroups. zero32: `zwords` int32 words per image that later launches accumulate into, cleared by the
// first tile of every image (nullptr: nothing to clear)
__global__ void __launch_bounds__(CC_THREADS) k_cc_tile(CcSrc s, int* __restrict__ par, int* __restrict__ ta, int* __restrict__ tot,
                                                        int* __restrict__ zero32, int zwords, int N, int H, int W, int tiles_x,
                                                        int tiles_y, int conn) {
    __shared__ int lp[CC_PIX];
    __shared__ int la[CC_PIX];
    __shared__ unsigned long long rows[CC_TILE];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const unsigned per = (unsigned)tiles_x * (unsigned)tiles_y;
    const unsigned q = blockIdx.x / per, t = blockIdx.x % per;
    const int ty = (int)(t / (unsigned)tiles_x), tx = (int)(t % (unsigned)tiles_x);
    const int n = (int)(q % (unsigned)N), mode = s.mode + (int)(q / (unsigned)N);
    const size_t HW = (size_t)H * W, src = (size_t)n * HW, dst = (size_t)q * HW;
    const int x = tx * CC_TILE + lane, y0 = ty * CC_TILE;
    if (zero32 && t == 0 && q < (unsigned)N && tid < zwords) zero32[(size_t)n * zwords + tid] = 0;
    // the mask, row by row; a pixel's first parent is the start of its horizontal run
    for (int k = 0; k < CC_ROWS; ++k) {
        const int r = wave + 4 * k, y = y0 + r;
        const bool f = y < H && x < W && cc_foreground(s, mode, src + (size_t)y * W + x, src);
        const unsigned long long m = __ballot(f);
        const unsigned long long below = ~m & ((1ull << lane) - 1ull);   // the background pixels to the left
        const int start = below ? 64 - __clzll(below) : 0;
        if (lane == 0) rows[r] = m;
        lp[r * CC_TILE + lane] = f ? r * CC_TILE + start : -1;
        la[r * CC_TILE + lane] = 0;
    }
    __syncthreads();
    // the unions with the row above. Left out: the pairs a neighbour in the same run makes (its run and the run above are the same two)
    for (int k = 0; k < CC_ROWS; ++k) {
        const int r = wave + 4 * k;
        if (r == 0) continue;
        const unsigned long long m = rows[r], up = rows[r - 1];
        if (!((m >> lane) & 1)) continue;
        const bool u = (up >> lane) & 1, l = lane > 0 && ((m >> (lane - 1)) & 1), ul = lane > 0 && ((up >> (lane - 1)) & 1);
        const bool rt = lane < 63 && ((m >> (lane + 1)) & 1), ur = lane < 63 && ((up >> (lane + 1)) & 1);
        const int i = r * CC_TILE + lane;
        if (u) {
            if (!(l && ul)) cc_lds_union(lp, i, i - CC_TILE);
        } else if (conn == 8) {
            if (ul && !l) cc_lds_union(lp, i, i - CC_TILE - 1);
            if (ur && !rt) cc_lds_union(lp, i, i - CC_TILE + 1);
        }
    }
    __syncthreads();
    // every pixel's tile root goes out as an image index; the first pixel of a run adds the run to its root's area and edge flag
    for (int k = 0; k < CC_ROWS; ++k) {
        const int r = wave + 4 * k, y = y0 + r;
        if (y >= H || x >= W) continue;
        const unsigned long long m = rows[r];
        const bool f = (m >> lane) & 1;
        const size_t g = dst + (size_t)y * W + x;
        int parent = 0;
        if (f) {
            const int root = cc_lds_find(lp, r * CC_TILE + lane);
            parent = (y0 + (root >> 6)) * W + tx * CC_TILE + (root & 63) + 1;
            if (lane == 0 || !((m >> (lane - 1)) & 1)) {
                const unsigned long long rest = ~(m >> lane);
                const int len = rest ? __ffsll((long long)rest) - 1 : 64;
                const bool edge = y == 0 || y == H - 1 || x == 0 || x + len - 1 == W - 1;
                atomicAdd(&la[root], len);
                if (edge) atomicOr(&la[root], CC_EDGE);
            }
        }
        par[g] = parent;
        if (tot) tot[g] = 0;
    }
    __syncthreads();
    if (!ta) return;   // (the pair count wants the roots alone)
    for (int k = 0; k < CC_ROWS; ++k) {
        const int r = wave + 4 * k, y = y0 + r, i = r * CC_TILE + lane;
        if (y >= H || x >= W) continue;
        ta[dst + (size_t)y * W + x] = lp[i] == i ? la[i] : 0;   // (a background pixel holds -1)
    }
}

// grid: planes * groups_y * groups_x workgroups, a group = 2^level x 2^level tiles
__global__ void __launch_bounds__(CC_THREADS) k_cc_merge(int* __restrict__ par, int H, int W, int groups_x, int groups_y, int level, int conn) {
    const int tid = threadIdx.x;
    const unsigned per = (unsigned)groups_x * (unsigned)groups_y;
    const unsigned q = blockIdx.x / per, t = blockIdx.x % per;
    const int gy = (int)(t / (unsigned)groups_x), gx = (int)(t % (unsigned)groups_x);
    int* p = par + (size_t)q * ((size_t)H * W);
    const long size = (long)CC_TILE << level, half = size >> 1;
    const long x0l = gx * size, y0l = gy * size;   // (< W, < H: the grid holds no empty group)
    const int x0 = (int)x0l, y0 = (int)y0l;
    const int x1 = (int)(x0l + size < W ? x0l + size : W), y1 = (int)(y0l + size < H ? y0l + size : H);
    const long xb = x0l + half, yb = y0l + half;
    if (xb < W) {   // the vertical border: columns xb - 1 | xb, the group's rows
        for (int y = y0 + tid; y < y1; y += CC_THREADS) {
            const int a = y * W + (int)xb - 1, b = a + 1;
            if (!p[a]) continue;
            if (p[b]) cc_union(p, a, b);
            if (conn == 8) {
                if (y + 1 < y1 && p[b + W]) cc_union(p, a, b + W);
                if (y - 1 >= y0 && p[b - W]) cc_union(p, a, b - W);
            }
        }
    }
    if (yb < H) {   // the horizontal border: rows yb - 1 | yb, the group's columns
        for (int x = x0 + tid; x < x1; x += CC_THREADS) {
            const int a = ((int)yb - 1) * W + x, b = a + W;
            if (!p[a]) continue;
            if (p[b]) cc_union(p, a, b);
            if (conn == 8) {
                if (x + 1 < x1 && p[b + 1]) cc_union(p, a, b + 1);
                if (x - 1 >= x0 && p[b - 1]) cc_union(p, a, b - 1);
            }
        }
    }
}

// grid: ceil(planes * HW / 256). lab may be the array ta: a pixel's thread alone reads and then writes that element
__global__ void __launch_bounds__(CC_THREADS) k_cc_flatten(const int* __restrict__ par, const int* ta, int* lab, int* __restrict__ tot,
                                                           unsigned HW, size_t total) {
    const size_t g = (size_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (g >= total) return;
    const size_t base = g - g % HW;
    const int t = ta[g];
    int v = par[g], label = 0;
    if (v) {
        int r = (int)(g - base);
        while (v - 1 != r) {
            r = v - 1;
            v = par[base + (size_t)r];
        }
        label = r + 1;
        if (t) {
            atomicAdd(&tot[base + (size_t)r], t & CC_AREA);
            if (t & CC_EDGE) atomicOr(&tot[base + (size_t)r], CC_EDGE);
        }
    }
    lab[g] = label;
}

__global__ void __launch_bounds__(CC_THREADS) k_cc_gather_label(const int* __restrict__ lab, const int* __restrict__ tot,
                                                                int32_t* __restrict__ area, uint8_t* __restrict__ edge, unsigned HW,
                                                                size_t total) {
    const size_t g = (size_t)blockIdx.x * CC_THREADS + threadIdx.x;
    if (g >= total) return;
    const int l = lab[g];
    const int t = l ? tot[g - g % HW + (size_t)(l - 1)] : 0;
    if (area) area[g] = t & CC_AREA;
    if (edge) edge[g] = (t & CC_EDGE) ? 1 : 0;
}

// grid: N * ceil(HW / 256): a workgroup stays inside one image. lab1 / lab2 nullptr: that labelling was skipped. stats [N][6] is cleared
// by the first tile launch; with both labellings skipped this launch writes the zeros
__global__ void __launch_bounds__(CC_THREADS) k_cc_gather_filter(const unsigned* prob, float thr, const int* __restrict__ lab1,
                                                                 const int* __restrict__ tot1, const int* __restrict__ lab2,
                                                                 const int* __restrict__ tot2, int min_area, int max_hole, unsigned* out,
                                                                 unsigned long long* __restrict__ stats, unsigned HW, unsigned blocks_per) {
    __shared__ int cnt[6];
    const int tid = threadIdx.x;
    const unsigned n = blockIdx.x / blocks_per, i = (blockIdx.x % blocks_per) * CC_THREADS + tid;
    const size_t base = (size_t)n * HW, g = base + i;
    if (tid < 6) cnt[tid] = 0;
    __syncthreads();
    bool c[6] = {false, false, false, false, false, false};
    if (i < HW) {
        const unsigned bits = prob[g];
        bool removed = false, filled = false;
        if (lab1) {
            const int l = lab1[g];
            if (l) {
                removed = (tot1[base + (size_t)(l - 1)] & CC_AREA) < min_area;
                c[0] = (unsigned)l == i + 1;
                c[1] = c[0] && removed;
                c[2] = removed;
            }
        }
        if (lab2) {
            const int l = lab2[g];
            if (l) {
                const int t = tot2[base + (size_t)(l - 1)];
                const bool hole = !(t & CC_EDGE);
                filled = hole && (t & CC_AREA) <= max_hole;
                c[3] = hole && (unsigned)l == i + 1;
                c[4] = c[3] && filled;
                c[5] = filled;
            }
        }
        out[g] = filled ? 0x3f800000u : removed ? 0u : bits;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        const int w = __popcll(__ballot(c[k]));
        if ((tid & 63) == 0 && w) atomicAdd(&cnt[k], w);
    }
    __syncthreads();
    if (stats && tid < 6) {
        if (lab1 || lab2) {
            if (cnt[tid]) atomicAdd(&stats[(size_t)n * 6 + tid], (unsigned long long)cnt[tid]);
        } else if (blockIdx.x % blocks_per == 0) {
            stats[(size_t)n * 6 + tid] = 0;
        }
    }
}

// grid: 2 N * ceil(HW / 256); plane q = image q % N, the prediction's roots (q < N) or the truth's. cnt [N][4] = {cp, cy, any counted, -}
__global__ void __launch_bounds__(CC_THREADS) k_cc_pair_roots(const int* __restrict__ par, const int64_t* __restrict__ labels64,
                                                              int* __restrict__ cnt, unsigned N, unsigned HW, unsigned blocks_per) {
    __shared__ int c[2];
    const int tid = threadIdx.x;
    const unsigned q = blockIdx.x / blocks_per, i = (blockIdx.x % blocks_per) * CC_THREADS + tid;
    const unsigned n = q % N, which = q / N;
    if (tid < 2) c[tid] = 0;
    __syncthreads();
    bool root = false, counted = false;
    if (i < HW) {
        root = (unsigned)par[(size_t)q * HW + i] == i + 1;
        if (which == 0) {
            const int64_t lab = labels64[(size_t)n * HW + i];
            counted = lab == 0 || lab == 1;
        }
    }
    const int wr = __popcll(__ballot(root)), wc = __ballot(counted) != 0;
    if ((tid & 63) == 0) {
        if (wr) atomicAdd(&c[0], wr);
        if (wc) atomicOr(&c[1], 1);
    }
    __syncthreads();
    if (tid == 0) {
        if (c[0]) atomicAdd(&cnt[(size_t)n * 4 + which], c[0]);
        if (c[1]) atomicOr(&cnt[(size_t)n * 4 + 2], 1);
    }
}
// one workgroup: acc[0..3] += {sum cp, sum cy, sum |cp - cy|, images with a counted pixel}
__global__ void __launch_bounds__(CC_THREADS) k_cc_pair_final(const int* __restrict__ cnt, unsigned long long* acc, int N) {
    __shared__ unsigned long long s[4];
    const int tid = threadIdx.x;
    if (tid < 4) s[tid] = 0;
    __syncthreads();
    unsigned long long v[4] = {0, 0, 0, 0};
    for (int n = tid; n < N; n += CC_THREADS) {
        const int cp = cnt[(size_t)n * 4], cy = cnt[(size_t)n * 4 + 1];
        v[0] += (unsigned long long)cp;
        v[1] += (unsigned long long)cy;
        v[2] += (unsigned long long)(cp > cy ? cp - cy : cy - cp);
        v[3] += (unsigned long long)(cnt[(size_t)n * 4 + 2] & 1);
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (v[k]) atomicAdd(&s[k], v[k]);
    __syncthreads();
    if (tid < 4) acc[tid] = acc[tid] + s[tid];
}

static int cc_tiles(int n) { return (n + CC_TILE - 1) / CC_TILE; }
int cc_levels(int H, int W) {
    const int t = cc_tiles(H) > cc_tiles(W) ? cc_tiles(H) : cc_tiles(W);
    int l = 0;
    while ((1 << l) < t) ++l;
    return l;
}
size_t cc_ws_bytes(int N, int H, int W) { return (size_t)N * H * W * 20 + (size_t)N * 16; }

// one labelling of `planes` masks: the tile launch, cc_levels merge launches and, with lab, the flatten launch
static void cc_run(const CcSrc& s, int planes, int conn, int* par, int* ta, int* lab, int* tot, int* zero32, int zwords, int N, int H, int W,
                   hipStream_t st) {
    const int tx = cc_tiles(W), ty = cc_tiles(H), levels = cc_levels(H, W);
    hipLaunchKernelGGL(k_cc_tile, dim3((unsigned)((size_t)planes * tx * ty)), dim3(CC_THREADS), 0, st, s, par, ta, tot, zero32, zwords, N, H, W,
                       tx, ty, conn);
    for (int m = 1; m <= levels; ++m) {
        const int gx = (tx + (1 << m) - 1) >> m, gy = (ty + (1 << m) - 1) >> m;
        hipLaunchKernelGGL(k_cc_merge, dim3((unsigned)((size_t)planes * gx * gy)), dim3(CC_THREADS), 0, st, par, H, W, gx, gy, m, conn);
    }
    if (lab) {
        const size_t total = (size_t)planes * H * W;
        hipLaunchKernelGGL(k_cc_flatten, dim3((unsigned)((total + CC_THREADS - 1) / CC_THREADS)), dim3(CC_THREADS), 0, st, par, ta, lab, tot,
                           (unsigned)(H * W), total);
    }
}

hipError_t cc_label(const float* prob, float threshold, int connectivity, int invert, int32_t* labels, int32_t* area, uint8_t* edge, void* ws,
                    int N, int H, int W, hipStream_t st) {
    const size_t total = (size_t)N * H * W;
    int* par = (int*)ws;
    int* tot = par + total;
    const CcSrc s = {prob, nullptr, nullptr, nullptr, threshold, 0, invert ? CC_INV : CC_FG};
    cc_run(s, N, connectivity, par, labels, labels, tot, nullptr, 0, N, H, W, st);
    if (area || edge)
        hipLaunchKernelGGL(k_cc_gather_label, dim3((unsigned)((total + CC_THREADS - 1) / CC_THREADS)), dim3(CC_THREADS), 0, st, labels, tot, area,
                           edge, (unsigned)(H * W), total);
    return hipGetLastError();
}

hipError_t cc_filter(const float* prob, float threshold, int connectivity, int min_area, int max_hole, float* out, int64_t* stats, void* ws,
                     int N, int H, int W, hipStream_t st) {
    const size_t total = (size_t)N * H * W;
    int* par = (int*)ws;
    int *lab1 = par + total, *tot1 = lab1 + total, *lab2 = tot1 + total, *tot2 = lab2 + total;
    const bool do1 = min_area > 1, do2 = max_hole > 0;
    int* zero = (int*)stats;   // [N][6] int64 = 12 int32 words per image
    if (do1) {
        const CcSrc s = {prob, nullptr, nullptr, nullptr, threshold, 0, CC_FG};
        cc_run(s, N, connectivity, par, lab1, lab1, tot1, zero, 12, N, H, W, st);
        zero = nullptr;
    }
    if (do2) {
        const CcSrc s = {prob, nullptr, do1 ? lab1 : nullptr, tot1, threshold, min_area, CC_HOLES};
        cc_run(s, N, connectivity == 8 ? 4 : 8, par, lab2, lab2, tot2, zero, 12, N, H, W, st);
    }
    const unsigned HW = (unsigned)(H * W), per = (HW + CC_THREADS - 1) / CC_THREADS;
    hipLaunchKernelGGL(k_cc_gather_filter, dim3((unsigned)N * per), dim3(CC_THREADS), 0, st, (const unsigned*)prob, threshold,
                       do1 ? lab1 : (const int*)nullptr, tot1, do2 ? lab2 : (const int*)nullptr, tot2, min_area, max_hole, (unsigned*)out,
                       (unsigned long long*)stats, HW, per);
    return hipGetLastError();
}

hipError_t cc_pair_count(const float* prob, float threshold, const int64_t* labels64, int connectivity, unsigned long long* acc, void* ws, int N,
                         int H, int W, hipStream_t st) {
    const size_t total = (size_t)N * H * W;
    int* par = (int*)ws;           // two planes per image: the prediction's parents, then the truth's
    int* cnt = par + 5 * total;
    const CcSrc s = {prob, labels64, nullptr, nullptr, threshold, 0, CC_PRED};
    cc_run(s, 2 * N, connectivity, par, nullptr, nullptr, nullptr, cnt, 4, N, H, W, st);
    const unsigned HW = (unsigned)(H * W), per = (HW + CC_THREADS - 1) / CC_THREADS;
    hipLaunchKernelGGL(k_cc_pair_roots, dim3(2u * (unsigned)N * per), dim3(CC_THREADS), 0, st, par, labels64, cnt, (unsigned)N, HW, per);
    hipLaunchKernelGGL(k_cc_pair_final, dim3(1), dim3(CC_THREADS), 0, st, cnt, acc, N);
    return hipGetLastError();
}
