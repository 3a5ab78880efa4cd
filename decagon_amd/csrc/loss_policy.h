// The cost as a policy of the decoder backward kernels (train.hip, gradseg.hip).
//
// Both costs of decagon/deep/optimizer.py are sums over the batch's pairs of a function of the
// positive score pos_p and the negative score neg_p, so the backward needs of the cost only
//   a_p = −∂cost/∂pos_p   and   b_p = +∂cost/∂neg_p.
// With M = L·G·L (L = diag(l)), u_p / un_p the positive / negative row and v_p the column:
//   the positive row u_p gets   −a_p·M·v_p
//   the negative row un_p gets  +b_p·M·v_p
//   grad_cols[p] = Mᵀ·(b_p·un_p − a_p·u_p)
//   dM           = Σ_p (b_p·un_p − a_p·u_p)·v_pᵀ
// and dG, dl, dG_diag follow from dM by the formulas in train.hip and gradseg.hip.
//
//   hinge  (_hinge_loss, optimizer.py:116-120)  cost = Σ_p relu(neg_p − (pos_p − margin))
//          a_p = b_p = [neg_p − (pos_p − margin) > 0]: a mask, so the kernels select instead
//          of multiplying (HingeLoss below compiles to the arithmetic they had before the
//          policy existed).
//   xent   (_xent_loss, optimizer.py:122-127)   cost = Σ_p softplus(−pos_p) + w·Σ_p softplus(neg_p)
//          a_p = σ(−pos_p),  b_p = w·σ(neg_p),  w = neg_sample_weights.
//          σ(−pos) is computed directly: 1 − σ(pos) cancels to zero from pos ≈ 17 on, where
//          the true coefficient is still 4e-8 of a gradient that is all that size.
//
// A policy has a value type Coef (the hinge: the mask itself, a bool) and static functions
//   coef(pos, neg, param, ok) → Coef   ok: the pair's indices lie inside the tables; a pair that
//                                      is not ok has a_p = b_p = 0
//   live(cf)          the pair contributes (a_p or b_p is not zero)
//   diff(cf, un, u)   b·un − a·u, one element
//   pos_row(cf, mv)   −a·mv        neg_row(cf, mv)  +b·mv
//   shfl(cf, src)     lane src's Coef (the dM kernels read a pair's once and pass it round)
//   a(cf), b(cf)      the two coefficients (policies with kCoef publish them)
#pragma once
#include "common.h"

namespace dg {

// σ(x) in fp32 without overflow: one expf of a non-positive argument serves both branches.
__device__ __forceinline__ float sigmoid_f32(float x) {
    const float e = expf(-fabsf(x));
    return (x >= 0.f ? 1.0f : e) / (1.0f + e);
}

struct HingeLoss {
    static constexpr bool kCoef = false;  // (a_p, b_p) are the mask: nothing to publish
    using Coef = bool;
    static __device__ __forceinline__ Coef coef(float pos, float neg, float margin, bool ok) {
        const float z = neg - (pos - margin);
        return ok && z > 0.f;
    }
    static __device__ __forceinline__ bool live(Coef act) { return act; }
    static __device__ __forceinline__ float diff(Coef, float un, float u) { return un - u; }
    static __device__ __forceinline__ float pos_row(Coef, float mv) { return -mv; }
    static __device__ __forceinline__ float neg_row(Coef, float mv) { return mv; }
    static __device__ __forceinline__ Coef shfl(Coef act, int src) { return __shfl((int)act, src) != 0; }
    static __device__ __forceinline__ float a(Coef act) { return act ? 1.0f : 0.f; }
    static __device__ __forceinline__ float b(Coef act) { return act ? 1.0f : 0.f; }
};

struct XentLoss {
    static constexpr bool kCoef = true;
    struct Coef {
        float a, b;
    };
    static __device__ __forceinline__ Coef coef(float pos, float neg, float w, bool ok) {
        return Coef{ok ? sigmoid_f32(-pos) : 0.f, ok ? w * sigmoid_f32(neg) : 0.f};
    }
    static __device__ __forceinline__ bool live(const Coef& c) { return c.a != 0.f || c.b != 0.f; }
    static __device__ __forceinline__ float diff(const Coef& c, float un, float u) { return c.b * un - c.a * u; }
    static __device__ __forceinline__ float pos_row(const Coef& c, float mv) { return -(c.a * mv); }
    static __device__ __forceinline__ float neg_row(const Coef& c, float mv) { return c.b * mv; }
    static __device__ __forceinline__ Coef shfl(const Coef& c, int src) {
        return Coef{__shfl(c.a, src), __shfl(c.b, src)};
    }
    static __device__ __forceinline__ float a(const Coef& c) { return c.a; }
    static __device__ __forceinline__ float b(const Coef& c) { return c.b; }
};

}  // namespace dg
