// Launch prototype of the one-launch batch loader (affine_patches.hip; rsu.h rsu_affine_patches).
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
