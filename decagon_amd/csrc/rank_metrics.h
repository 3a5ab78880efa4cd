// The arithmetic of the rank metrics shared by eval.hip (one relation per call) and evalseg.hip
// (all relations of an edge type per call): the score an edge is ranked by, and the double sums
// over a relation's per-positive count records.  One definition, so the two entry points agree
// bit for bit.
#pragma once
#include "common.h"

namespace dg {

// The score each edge is ranked by (mode, dg_rank_metrics_ex_f32), from its logit x:
//   DG_RANK_LOGIT      x itself (float)
//   DG_RANK_SIGMOID64  main.py:51-52,60,70,81 under numpy 1.14 (requirements.txt:14): rec is
//                      TF's float32, so np.exp(-x) runs in float32 (glibc expf: correctly
//                      rounded — computed here as (float)exp((double)-x)), `1 + e` and `1. / …`
//                      promote to float64, then np.nan_to_num.  Saturates: x > ≈36.7 → 1.0,
//                      x < ≈-88.7 → 0.0 (float32 exp overflows), so large logits tie.
//   DG_RANK_SIGMOID32  MathUtils.sigmoid on the float32 decoder output array
//                      (DecagonAccuracyEvaluator.py:123): every step float32 (x > ≈16.6 → 1.0)
__device__ __forceinline__ double score_key(float v, int mode) {
    double k = v;
    if (mode != DG_RANK_LOGIT) {
        const float e = (float)exp(-(double)v);
        if (mode == DG_RANK_SIGMOID64) {
            k = 1.0 / (1.0 + (double)e);
        } else {
            const float one = 1.0f;
            k = (double)(one / (one + e));
        }
        if (k != k) k = 0.0;  // np.nan_to_num (only a NaN logit gets here)
    }
    return k;
}

// The 8-int record of one positive from its six counts (the layout rank_reduce_block reads):
// {#neg < s, #neg == s, #pos >= s, #all >= s, #all > s, #pos > s, #pos before it with == s, -}
__device__ __forceinline__ void rank_record(int* o, int lt_neg, int eq_neg, int ge_pos, int gt_pos, int eq_before,
                                            int gt_neg) {
    o[0] = lt_neg;
    o[1] = eq_neg;
    o[2] = ge_pos;
    o[3] = ge_pos + eq_neg + gt_neg;
    o[4] = gt_pos + gt_neg;
    o[5] = gt_pos;
    o[6] = eq_before;
}

// out[0..2] = {AUROC, AUPRC, AP@k} of the P records at `counts`, by one 256-thread workgroup:
// thread t sums positives t, t + 256, ... in double, then a fixed tree — deterministic.
__device__ __forceinline__ void rank_reduce_block(const int* counts, int P, int N, int k, double* out,
                                                  double (*red)[256]) {
    double au = 0.0, ap = 0.0, apk = 0.0;
    for (int i = threadIdx.x; i < P; i += 256) {
        const int* c = counts + (int64_t)i * 8;
        au += (double)c[0] + 0.5 * (double)c[1];
        ap += (double)c[2] / (double)c[3];
        const int rank = c[4] + c[6];
        if (rank < k) apk += ((double)(c[5] + c[6]) + 1.0) / ((double)rank + 1.0);
    }
    red[0][threadIdx.x] = au;
    red[1][threadIdx.x] = ap;
    red[2][threadIdx.x] = apk;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int q = 0; q < 3; ++q) red[q][threadIdx.x] += red[q][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = N > 0 && P > 0 ? red[0][0] / ((double)P * (double)N) : __builtin_nan("");
        out[1] = P > 0 ? red[1][0] / (double)P : __builtin_nan("");
        out[2] = P > 0 ? red[2][0] / (double)(P < k ? P : k) : 0.0;
    }
}

}  // namespace dg
