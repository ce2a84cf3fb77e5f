// What the sweeps with raw edge features share (spmm_softmax_edge.hip, spmm_pna_edge.hip): the load of an edge's K floats (load_ef), a
// lane's KP x VEC slice of the transposed weight (load_slice), the edge term's chain (edge_chain), the persistent backward's grid
// (edge_bwd_blocks) and the ladder over the padded K (dispatch_kp).
#pragma once
#include "sweep.h"

// NOTE: the pragma below is at file scope, so it holds for the REST of any translation unit that includes this header (as smx.h's does).
// That is intended: every product of the chain is rounded on its own and every fused multiply-add is written out, so a forward and its
// backward form the same bits.  Include it last.
#pragma clang fp contract(off)

namespace bot {

constexpr int kEdgeMaxK = 16;
constexpr int64_t kEdgeBwdBlockCap = 1024;  // workgroups of the backward over all feature tiles: two rounds of two per CU
constexpr int kEdgeBwdItemsPerGroup = 4;    // a group sees at least this many items before another workgroup is opened

// The ef row of one edge: e[j] for j < K, zeros behind it
template <int KP>
__device__ __forceinline__ void load_ef(float (&e)[KP], const float* p, int K, bool k4) {
    if (k4) {
#pragma unroll
        for (int j = 0; j < KP; j += 4) {
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (j < K) v = *reinterpret_cast<const float4*>(p + j);
            e[j] = v.x, e[j + 1] = v.y, e[j + 2] = v.z, e[j + 3] = v.w;
        }
    } else {
#pragma unroll
        for (int j = 0; j < KP; ++j) e[j] = j < K ? p[j] : 0.f;
    }
}

// A lane's slice of wt [K, F] and of bias for the VEC columns from `off`: w[j] zeros for j >= K, b zeros without a bias
template <int KP, int VEC>
__device__ __forceinline__ void load_slice(float (&w)[KP][VEC], float (&b)[VEC], const float* wt, const float* bias, int K, int F, int off) {
#pragma unroll
    for (int j = 0; j < KP; ++j) {
#pragma unroll
        for (int t = 0; t < VEC; ++t) w[j][t] = 0.f;
        if (j < K) vload<VEC>(w[j], wt + (int64_t)j * F + off);
    }
#pragma unroll
    for (int t = 0; t < VEC; ++t) b[t] = 0.f;
    if (bias) vload<VEC>(b, bias + off);
}

// The edge term of the contracts: ef[e,0] wt[0,f], then fmaf(ef[e,j], wt[j,f], .) for j = 1 .. in index order: a rounded product, then
// a chain of fused multiply-adds (the padding's zeros add +0)
template <int KP, int VEC>
__device__ __forceinline__ float edge_chain(const float (&e)[KP], const float (&w)[KP][VEC], int t) {
    float s = e[0] * w[0][t];
#pragma unroll
    for (int j = 1; j < KP; ++j) s = fmaf(e[j], w[j][t], s);
    return s;
}

// grid.x of the backward: a pure function of the plan's item count and the tiling, capped; never of the device
static int64_t edge_bwd_blocks(int64_t n_items, int lanes, int64_t n_tiles) {
    const int64_t per_block = (int64_t)(kBlock / lanes) * kEdgeBwdItemsPerGroup;
    const int64_t cap = kEdgeBwdBlockCap / n_tiles > 1 ? kEdgeBwdBlockCap / n_tiles : 1;
    const int64_t want = (n_items + per_block - 1) / per_block;
    return want < 1 ? 1 : (want > cap ? cap : want);
}

// The padded K of the instance that serves K: the one place that states the ladder
__host__ __device__ constexpr int edge_kp(int K) { return K <= 4 ? 4 : (K <= 8 ? 8 : 16); }

template <class L>
static void dispatch_kp(const L& l, int K, int F, int vec) {
    const int kp = edge_kp(K);
    if (kp == 4) dispatch_sweep(typename L::template At<4>{l}, F, vec);
    else if (kp == 8) dispatch_sweep(typename L::template At<8>{l}, F, vec);
    else dispatch_sweep(typename L::template At<16>{l}, F, vec);
}

}  // namespace bot
