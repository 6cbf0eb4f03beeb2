// bow_score.h -- the per-pair arithmetic of DBoW2 GeneralScoring::score (ScoringObject.cpp:23-313),
// shared by bow_db_score_kernel (bow.hip: one thread walks a pair) and the keyframe database on the
// device (kfdb.hip: one wave per pair).  Both add the terms in ascending word order, so both give
// the same double; the build's -ffp-contract=off keeps every expression as it is written here.
//   scoring 0 L1, 1 L2, 2 chi-square, 3 KL, 4 Bhattacharyya, 5 dot product
#pragma once

#include <hip/hip_runtime.h>

namespace orbgpu {
namespace bowscore {

// log(DBL_EPSILON), KL's stand-in for a word the keyframe lacks
__device__ __forceinline__ double kl_log_eps() { return log(2.220446049250313080847e-16); }

// The term of a word both vectors hold (vi the query's value, wi the keyframe's).  *add is false
// where the reference adds nothing for this pair of values.
__device__ __forceinline__ double common_term(int scoring, double vi, double wi, bool* add) {
    *add = true;
    switch (scoring) {
        case 0: return fabs(vi - wi) - fabs(vi) - fabs(wi);  // L1
        case 1: case 5: return vi * wi;                      // L2, dot product
        case 2:                                              // chi-square
            if (vi + wi != 0.0) return vi * wi / (vi + wi);
            *add = false;
            return 0.0;
        case 3:  // KL
            if (vi != 0 && wi != 0) return vi * log(vi / wi);
            *add = false;
            return 0.0;
        default: return sqrt(vi * wi);  // Bhattacharyya
    }
}

// KL's term of a query word the keyframe lacks
__device__ __forceinline__ double kl_query_only_term(double vi, double log_eps) { return vi * (log(vi) - log_eps); }

// the sum of the terms -> the score
__device__ __forceinline__ double finish(int scoring, double s) {
    if (scoring == 0) return -s / 2.0;
    if (scoring == 1) return s >= 1 ? 1.0 : 1.0 - sqrt(1.0 - s);
    if (scoring == 2) return 2. * s;
    return s;
}

}  // namespace bowscore
}  // namespace orbgpu
