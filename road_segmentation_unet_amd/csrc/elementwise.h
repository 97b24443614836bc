// Launch prototypes of the bandwidth-bound kernels (elementwise.hip).
#pragma once
#include "rsu_common.h"

struct PackParams {
    int nchunks, ntap, ntiles;  // packed dims: [nchunks][ntap][ntiles][64][8]
    int rows;                   // real output rows (channels)
    int nseg, seg_c[3];         // K segments (concat sources), real channel counts
    long s_tap, s_row, s_k;     // source strides (elements)
    int flip;                   // read source tap (ntap-1-tap)
};

hipError_t ew_color_adjust(const float* x, const float* w, const float* b, void* out16, long npix, float keep, unsigned key, hipStream_t st);
hipError_t ew_scale_bf16(void* x, long n, float s, hipStream_t st);
hipError_t ew_dropout(const void* x, void* y, long n, float keep, unsigned key, hipStream_t st);
hipError_t ew_scatter_first_grads(const float* tmp, float* dw1, float* gxc, int Cout, hipStream_t st);
hipError_t ew_maxpool_fwd(const void* x, void* y, void* code, int N, int H, int W, int C, float keep, unsigned key, hipStream_t st);
hipError_t ew_pool_skip_relu_bwd(const void* yact, const void* code, const void* dpool, const void* dskip, void* dz, int N, int H, int W, int C, int Hs, int Ws,
                                 float keep, unsigned key, hipStream_t st);
int ew_colsum_blocks(long npix, int C);
hipError_t ew_colsum(const void* dz, float* db, float* ws, long npix, int C, hipStream_t st);
// out2 (optional): n2 more float4 items behind the taps of every slab, reduced into out2 by the same launch
hipError_t ew_reduce_slabs(const float* slab, float* out, float* out2, int n2, int nsplit, long slab_elems, int ntap, int CsOut, int cs_off, int cs_cnt,
                           int CfOut, hipStream_t st);
// grouped form: one launch reduces the slabs of several weight-gradient jobs (device-resident job table)
struct ReduceJob {
    const float* slab; float* out; float* out2;
    long slab_elems;
    int n2, nsplit, ntap, CsOut, cs_off, cs_cnt, CfOut;
    int block_begin, wide, pad_;
};
int ew_reduce_job_blocks(ReduceJob& j);   // sets j.wide, returns the workgroups the job needs
hipError_t ew_reduce_slabs_many(const ReduceJob* jobs_dev, int njobs, int total_blocks, hipStream_t st);
hipError_t ew_color_adjust_bwd(const float* gx, const float* w1, float* dW0, float* db0, int Cout, float scale, int accumulate, hipStream_t st);
hipError_t ew_pack(const float* src, void* dst, const PackParams& pp, hipStream_t st);
struct PackJob { PackParams pp; const float* src; bf16_t* dst; int block_start; int pad_; };
hipError_t ew_pack_many(const PackJob* jobs_dev, int njobs, int total_blocks, hipStream_t st);
int ew_pack_blocks(const PackParams& pp);
hipError_t ew_extract_tiles(const float* imgs, float* tiles, int H, int S, int P, int stride, int pps, long t0, long ntiles, hipStream_t st);
hipError_t ew_overlap_add(const float* prob, float* acc, float* hits, int nimg, int H, int P, int stride, int pps, long t0, long ntiles, hipStream_t st);
hipError_t ew_overlap_finish(const float* acc, const float* hits, float* out, long n, hipStream_t st);
void ew_tile_grid(int H, int W, int P, int stride, int* ny, int* nx);
hipError_t ew_extract_tiles_rect(const float* imgs, float* tiles, int H, int W, int S, int P, int stride, long t0, long ntiles, hipStream_t st);
hipError_t ew_overlap_add_rect(const float* prob, float* acc, float* hits, int nimg, int H, int W, int P, int stride, long t0, long ntiles,
                               hipStream_t st);
hipError_t ew_block_label_rect(const float* mask, float* out, int nimg, int H, int W, int ps, float thr, hipStream_t st);
hipError_t ew_block_label(const float* mask, float* out, int64_t* labels, int nimg, int S, int ps, float thr, int mode, hipStream_t st);
hipError_t ew_confusion(const int64_t* pred, const int64_t* truth, long n, unsigned long long* counts, hipStream_t st);
