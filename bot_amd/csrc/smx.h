// The online-softmax arithmetic that spmm_softmax.hip, spmm_softmax_edge.hip (per column) and dot_attn.hip (per head) share: the
// exponential and the merge of two running states (M, Z, S[, Q]).  Every product is rounded on its own and every fused multiply-add is
// written out, so the sweeps, their chunks and their combine kernels run the same arithmetic and give the same bytes.  Below them, what
// the two per-column sweeps share behind the message m: the message's select, the arguments of the outputs (SmxArgs), where a group's
// state goes (BOT_SMX_FINISH_TILE: a chunk's raw state into the workspace, or the row's epilogue) and the long rows' combine (launch_smx_combine).
#pragma once
#include "common.h"
#include "sweep.h"

// NOTE: the pragma below is at file scope, so it holds for the REST of any translation unit that includes this header.  That is
// intended for its includers (spmm_softmax.hip, spmm_softmax_edge.hip, dot_attn.hip), which say so where they include it; include it last.
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

// relu(x) + eps written as a select, so that a NaN stays a NaN (fmaxf would drop it): the kernel and the tensor form (torch.relu) agree
__device__ __forceinline__ float smx_message(float x, bool relu, float eps) { return relu ? (x < 0.f ? 0.f : x) + eps : x; }

struct SmxArgs {
    const int32_t* indices;
    const int4* items;
    int64_t n_items;
    const float* x;
    int64_t ldx;
    const float* beta;
    int32_t F;
    int32_t relu;
    float eps;
    float* out;
    int64_t ldo;
    float* lse;
    int64_t ldl;
    float* q;
    int64_t ldq;
    float* ws;        // [3 or 4][n_slots, F]: the chunks' M, Z, S (, Q)
    int64_t plane;    // n_slots * F
};

// Where a group's state of one column tile goes, as the last statement of a sweep's loop over column tiles.  A chunk of a long row
// (it.slot >= 0) leaves the raw state in the workspace, folded by spmm_softmax_combine_kernel; a whole row gets its epilogue, zeros when it
// is empty.  In scope where it is used: SmxArgs a, RowItem it, ColTile<VEC, LANES, NCHUNK> tile, float M, Z, S, Q [NCHUNK][VEC], WQ.
// A macro and not a function: written as inlined functions the same statements compile to other code in spmm_softmax_kernel (another
// register assignment and schedule in all 30 instances), and that kernel's object code is held fixed; the text is in one place this way.
#define BOT_SMX_FINISH_TILE()                                                                       \
    if (it.slot >= 0) {                                                                             \
        float* w = a.ws + (int64_t)it.slot * a.F;                                                   \
        _Pragma("unroll") for (int c = 0; c < NCHUNK; ++c) if (tile.act[c]) {                       \
            vstore<VEC>(w + tile.off[c], M[c]);                                                     \
            vstore<VEC>(w + a.plane + tile.off[c], Z[c]);                                           \
            vstore<VEC>(w + 2 * a.plane + tile.off[c], S[c]);                                       \
            if constexpr (WQ) vstore<VEC>(w + 3 * a.plane + tile.off[c], Q[c]);                     \
        }                                                                                           \
        continue;                                                                                   \
    }                                                                                               \
    const bool some = it.beg < it.end; /* an empty row: zeros */                                    \
    _Pragma("unroll") for (int c = 0; c < NCHUNK; ++c) if (tile.act[c]) {                           \
        float o[VEC], l[VEC], qq[VEC];                                                              \
        _Pragma("unroll") for (int t = 0; t < VEC; ++t) {                                           \
            o[t] = some ? S[c][t] / Z[c][t] : 0.f;                                                  \
            l[t] = some ? M[c][t] + logf(Z[c][t]) : 0.f;                                            \
            qq[t] = some ? Q[c][t] / Z[c][t] : 0.f;                                                 \
        }                                                                                           \
        vstore<VEC>(a.out + (int64_t)it.row * a.ldo + tile.off[c], o);                              \
        vstore<VEC>(a.lse + (int64_t)it.row * a.ldl + tile.off[c], l);                              \
        if constexpr (WQ) vstore<VEC>(a.q + (int64_t)it.row * a.ldq + tile.off[c], qq);             \
    }

// The long rows' chunks folded in slot order with smx_merge, then the row's epilogue (spmm_softmax.hip: spmm_softmax_combine_kernel, with
// Q when a.q is there); the caller reads the launch status
void launch_smx_combine(const SmxArgs& a, const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, hipStream_t st);

}  // namespace bot
