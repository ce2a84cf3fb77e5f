// The online-softmax arithmetic that spmm_softmax.hip (per column) and dot_attn.hip (per head) share: the exponential and the merge of
// two running states (M, Z, S[, Q]).  Every product is rounded on its own and every fused multiply-add is written out, so the sweeps,
// their chunks and their combine kernels run the same arithmetic and give the same bytes.
#pragma once
#include "common.h"

// NOTE: the pragma below is at file scope, so it holds for the REST of any translation unit that includes this header.  That is
// intended for its two includers (spmm_softmax.hip, dot_attn.hip), which say so where they include it; include it last.
#pragma clang fp contract(off)

namespace bot {

// exp(t) for t <= 0 (and the few roundings above 0 the backward's arguments reach); NaN for a NaN or infinite t
__device__ __forceinline__ float smx_exp(float t) {
    const float hi = t * 1.442695041f;  // log2(e)
    float c = fmaf(-hi, 0.693145752f, t);  // t - hi ln 2: ln 2 in two pieces, the first with 12 trailing zero bits
    c = fmaf(-hi, 1.428606820e-6f, c);
    const float r = __builtin_amdgcn_exp2f(hi);
    return fmaf(r, c, r);
}

// (M, Z, S, Q) += (M2, Z2, S2, Q2): the sums of the side with the smaller maximum are rescaled by the one exponential
template <bool WQ>
__device__ __forceinline__ void smx_merge(float& M, float& Z, float& S, float& Q, float M2, float Z2, float S2, float Q2) {
    const float d = M2 - M;
    const float e = smx_exp(-fabsf(d));
    const bool up = d > 0.f;
    const float fo = up ? e : 1.f, fn = up ? 1.f : e;
    Z = fmaf(Z, fo, Z2 * fn);
    S = fmaf(S, fo, S2 * fn);
    if constexpr (WQ) Q = fmaf(Q, fo, Q2 * fn);
    M = up ? M2 : M;
}

}  // namespace bot
