// Launch prototypes of the one-launch batch loader (affine_patches.hip; rsu.h rsu_affine_patches, rsu_elastic_patches).
#pragma once
#include "rsu_common.h"

constexpr int AP_MAX_LAUNCH = 32;   // records per launch (rsu.h RSU_AFFINE_MAX_LAUNCH): they travel as kernel arguments
// one sample: rsu.h rsu_affine_t, field for field
struct ApRec {
    int image;
    float cy, cx;
    float m00, m01, m10, m11;
    int pad_;
};
// recs: a HOST pointer; cut into launches of at most AP_MAX_LAUNCH records on `st`
hipError_t ap_affine_patches(const float* images, const uint8_t* labels, const ApRec* recs, int nrec, int He, int Hl, int S, int P, float* x_out,
                             int64_t* labels_out, hipStream_t st);

constexpr int EP_MAX_LAUNCH = 32;   // records per launch (rsu.h RSU_ELASTIC_MAX_LAUNCH): 1.5 KB of kernel arguments
constexpr int EP_MAX_GRID = 16;     // cells per axis at most: a lattice of (16 + 3)^2 points, two floats each, in LDS
// one sample: rsu.h rsu_elastic_t, field for field (the launcher writes q = (float)(grid / (double)S) into the first padding word of its own copy)
struct EpRec {
    int image;
    float cy, cx;
    float m00, m01, m10, m11;
    float alpha;
    unsigned key;
    int grid;
    int pad_[2];
};
// recs: a HOST pointer, every grid in [1, EP_MAX_GRID]; cut into launches of at most EP_MAX_LAUNCH records on `st`
hipError_t ep_elastic_patches(const float* images, const uint8_t* labels, const EpRec* recs, int nrec, int He, int Hl, int S, int P, float* x_out,
                              int64_t* labels_out, hipStream_t st);
