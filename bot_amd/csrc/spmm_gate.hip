// Gated aggregation sweeps (include/bot_gnn.h "Gated aggregation") for gfx950: the per-channel sigmoid gate of Bresson & Laurent,
// "Residual Gated Graph ConvNets" (arXiv:1711.07553) - the GatedGCN of Dwivedi et al., "Benchmarking Graph Neural Networks"
// (arXiv:2003.00982), PyG's ResGatedGraphConv; bot_amd.nn.ResGatedGraphConv, `ops.gated_sum`.  The gate of an edge u -> w is a VECTOR
// that depends on both endpoints, so it splits neither into per-node scalars nor into a source-only message:
//   forward        num[w,f] = sum_j g_j v[u_j,f],  den[w,f] = sum_j g_j,  g_j = sigmoid(k[w,f] + q[u_j,f])      (rows = destinations: the CSC)
//                  out = num, or - normalised - num / (den + eps)
//   backward, dst  dk[w]    = sum_j ds_j,  ds_j = g'_j (v[u_j] a[w] + b[w])                                       (the CSC)
//   backward, src  dq[u]    = sum_j ds_j,  dv[u] = sum_j g_j a[w_j]                                               (rows = sources: the CSR)
// with a = dout (b absent), or - normalised - a = dout / (den + eps), b = -a out, formed by the caller with dense ops.
//
// The gate (gate_of): s = k + q, e = smx_exp(-|s|), g = (s >= 0 ? 1 : e) / (1 + e), gbar = (s >= 0 ? e : 1) / (1 + e), g' = g gbar.  Both
// quotients are true divisions and the complement is formed directly, never as 1 - g, so g' keeps a RELATIVE error bound in both tails;
// s = 0 gives g = gbar = 0.5, s >= 105 gives e = 0 (below the smallest denormal), g = 1, g' = 0, s <= -105 gives g = 0, g' = 0, bit for bit.
// One exponential and two divisions per gathered element; nothing is stored per edge, both backward sweeps form the gate again.
//
// The gather is the lane-group row sweep that sweep.h describes (walk_row), lane layout as in bot_spmm_max_f32.  The row a group owns
// (k of the destination, with a and b in the backward; q and v of the source) stays in registers across its neighbours.  The sums run in
// position order in registers; the chunks of a long row leave (num[, den]) - or their partial dk / dq / dv - in the workspace and are
// folded in slot order (spmm_gate_combine_kernel applies the division after the fold; the plain sums go through launch_sum_combine).
// Every product is rounded on its own and every fused multiply-add is written out (smx.h switches contraction off), so the chunks, the
// combine and the whole rows run the same arithmetic.  No atomics: the bytes repeat from call to call.
//
// HBM model (4-byte words), for the comparison with the sum sweep (bot_spmm_f32) at width 2F, which moves 4 [E (1 + 2F) + 2 n F]:
//   forward        4 [E (1 + 2F) + n_dst F (2 or 3)]        ids and the (q, v) row pair per edge; k read, out (and den) written per row
//   backward, dst  4 [E (1 + 2F) + n_dst F (3 or 4)]        the same gather; k, a (and b) read, dk written per row
//   backward, src  4 [E (1 + (2 or 3) F) + 4 n_src F]       ids and k, a (and b) of the destination per edge; q, v read, dq, dv written
// The layer passes q and v as the two column blocks of one [n_src, 2F] projection, so the pair of a neighbour is one contiguous row.
#include "sweep.h"

#include <cmath>
#include <initializer_list>

// (contraction off for the rest of this file: see above; gate_of lives in gate.h, shared with spmm_gate_edge.hip)
#include "gate.h"

namespace bot {

struct GateArgs {
    const int32_t* indices;
    const int4* items;
    int64_t n_items;
    const float* k;
    int64_t ldk;
    const float* q;
    int64_t ldq;
    const float* v;
    int64_t ldv;
    const float* a;  // backward: [n_dst, F]
    int64_t lda;
    const float* b;  // backward, normalised: [n_dst, F]
    int64_t ldb;
    int32_t F;
    float eps;
    float* o0;  // forward: out; backward dst: dk; backward src: dq (NULL: not asked for)
    int64_t ld0;
    float* o1;  // forward: den (normalised); backward src: dv (NULL: not asked for)
    int64_t ld1;
    float* ws;      // the long rows' chunks: planes of n_slots * F floats
    int64_t plane;  // n_slots * F
};

template <int VEC, int NCHUNK>
struct GatePair {
    float q[NCHUNK][VEC], v[NCHUNK][VEC];
};

template <int VEC, int NCHUNK>
struct GateTriple {
    float k[NCHUNK][VEC], a[NCHUNK][VEC], b[NCHUNK][VEC];
};

template <bool NORM, int VEC, int LANES, int NCHUNK>
__global__ __launch_bounds__(kBlock) void spmm_gate_kernel(GateArgs a) {
    constexpr int TILE = LANES * VEC * NCHUNK;
    const int lane = threadIdx.x % LANES;
    const int64_t item = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / LANES;
    if (item >= a.n_items) return;  // whole groups leave together
    const RowItem it = load_item<LANES>(a.items, item);
    for (int col0 = 0; col0 < a.F; col0 += TILE) {  // groups narrower than a wavefront have one tile
        const ColTile<VEC, LANES, NCHUNK> tile(col0, lane, a.F);
        float kv[NCHUNK][VEC], num[NCHUNK][VEC] = {}, den[NCHUNK][VEC] = {};
#pragma unroll
        for (int c = 0; c < NCHUNK; ++c) vload<VEC>(kv[c], a.k + (int64_t)it.row * a.ldk + tile.off[c]);
        walk_row<LANES, GatePair<VEC, NCHUNK>>(
            it.beg, it.end, lane, [&](int p, bool in) { return Edge{in ? a.indices[p] : 0, 0}; },
            [&](int s, int, GatePair<VEC, NCHUNK>& st, int) {
                const float* pq = a.q + (int64_t)s * a.ldq;
                const float* pv = a.v + (int64_t)s * a.ldv;
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c) {
                    vload<VEC>(st.q[c], pq + tile.off[c]);
                    vload<VEC>(st.v[c], pv + tile.off[c]);
                }
            },
            [&](int, int, const GatePair<VEC, NCHUNK>& st, int) {
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c)
#pragma unroll
                    for (int t = 0; t < VEC; ++t) {
                        const float g = gate_of(kv[c][t] + st.q[c][t]).g;
                        num[c][t] = fmaf(g, st.v[c][t], num[c][t]);
                        if constexpr (NORM) den[c][t] += g;
                    }
            });
        if (it.slot >= 0) {  // a chunk of a long row: the raw sums into the workspace
            float* w = a.ws + (int64_t)it.slot * a.F;
            tile.store(w, num);
            if constexpr (NORM) tile.store(w + a.plane, den);
            continue;
        }
        if constexpr (NORM) {
#pragma unroll
            for (int c = 0; c < NCHUNK; ++c)
#pragma unroll
                for (int t = 0; t < VEC; ++t) num[c][t] = num[c][t] / (den[c][t] + a.eps);  // an empty row: 0 / eps, or 0 / 0 -> see below
            if (it.beg == it.end) {
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c)
#pragma unroll
                    for (int t = 0; t < VEC; ++t) num[c][t] = 0.f;  // a select: an empty row is 0 whatever eps is
            }
            tile.store(a.o1 + (int64_t)it.row * a.ld1, den);
        }
        tile.store(a.o0 + (int64_t)it.row * a.ld0, num);
    }
}

// One thread per (long row, column) of the normalised forward: the chunks' num and den are added in slot order (= position order), then
// the row's division.  (A long row has at least two chunks and no chunk is empty.)
__global__ __launch_bounds__(kBlock) void spmm_gate_combine_kernel(GateArgs a, const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long) {
    const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gid >= n_long * a.F) return;
    const int64_t i = gid / a.F;
    const int c = (int)(gid - i * a.F);
    const int row = long_rows[i], p1 = long_ptr[i + 1];
    float num = 0.f, den = 0.f;
    for (int s = long_ptr[i]; s < p1; ++s) {
        const float* w = a.ws + (int64_t)s * a.F + c;
        num += w[0];
        den += w[a.plane];
    }
    a.o0[(int64_t)row * a.ld0 + c] = long_ptr[i] < p1 ? num / (den + a.eps) : 0.f;
    a.o1[(int64_t)row * a.ld1 + c] = den;
}

// Backward over the destinations: the forward's gather; the row owner holds k, a (and b) of its destination.
template <bool NORM, int VEC, int LANES, int NCHUNK>
__global__ __launch_bounds__(kBlock) void spmm_gate_bwd_dst_kernel(GateArgs a) {
    constexpr int TILE = LANES * VEC * NCHUNK;
    const int lane = threadIdx.x % LANES;
    const int64_t item = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / LANES;
    if (item >= a.n_items) return;  // whole groups leave together
    const RowItem it = load_item<LANES>(a.items, item);
    for (int col0 = 0; col0 < a.F; col0 += TILE) {
        const ColTile<VEC, LANES, NCHUNK> tile(col0, lane, a.F);
        float kv[NCHUNK][VEC], av[NCHUNK][VEC], bv[NCHUNK][VEC] = {}, acc[NCHUNK][VEC] = {};
#pragma unroll
        for (int c = 0; c < NCHUNK; ++c) {
            vload<VEC>(kv[c], a.k + (int64_t)it.row * a.ldk + tile.off[c]);
            vload<VEC>(av[c], a.a + (int64_t)it.row * a.lda + tile.off[c]);
            if constexpr (NORM) vload<VEC>(bv[c], a.b + (int64_t)it.row * a.ldb + tile.off[c]);
        }
        walk_row<LANES, GatePair<VEC, NCHUNK>>(
            it.beg, it.end, lane, [&](int p, bool in) { return Edge{in ? a.indices[p] : 0, 0}; },
            [&](int s, int, GatePair<VEC, NCHUNK>& st, int) {
                const float* pq = a.q + (int64_t)s * a.ldq;
                const float* pv = a.v + (int64_t)s * a.ldv;
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c) {
                    vload<VEC>(st.q[c], pq + tile.off[c]);
                    vload<VEC>(st.v[c], pv + tile.off[c]);
                }
            },
            [&](int, int, const GatePair<VEC, NCHUNK>& st, int) {
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c)
#pragma unroll
                    for (int t = 0; t < VEC; ++t) {
                        const Gate g = gate_of(kv[c][t] + st.q[c][t]);
                        const float m = NORM ? fmaf(st.v[c][t], av[c][t], bv[c][t]) : st.v[c][t] * av[c][t];
                        acc[c][t] = fmaf(g.g * g.gbar, m, acc[c][t]);
                    }
            });
        tile.store(sum_row(it, a.o0, a.ld0, a.ws, a.F), acc);
    }
}

// Backward over the sources: the row owner holds q (and v, for dq) of its source; per out-edge the destination's k, a (and b).
template <bool NORM, int VEC, int LANES, int NCHUNK>
__global__ __launch_bounds__(kBlock) void spmm_gate_bwd_src_kernel(GateArgs a) {
    constexpr int TILE = LANES * VEC * NCHUNK;
    const int lane = threadIdx.x % LANES;
    const int64_t item = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / LANES;
    if (item >= a.n_items) return;  // whole groups leave together
    const RowItem it = load_item<LANES>(a.items, item);
    const bool wq = a.o0 != nullptr, wv = a.o1 != nullptr;  // uniform over the launch
    for (int col0 = 0; col0 < a.F; col0 += TILE) {
        const ColTile<VEC, LANES, NCHUNK> tile(col0, lane, a.F);
        float qv[NCHUNK][VEC], vv[NCHUNK][VEC], dq[NCHUNK][VEC] = {}, dv[NCHUNK][VEC] = {};
#pragma unroll
        for (int c = 0; c < NCHUNK; ++c) {
            vload<VEC>(qv[c], a.q + (int64_t)it.row * a.ldq + tile.off[c]);
            vload<VEC>(vv[c], a.v + (int64_t)it.row * a.ldv + tile.off[c]);
        }
        walk_row<LANES, GateTriple<VEC, NCHUNK>>(
            it.beg, it.end, lane, [&](int p, bool in) { return Edge{in ? a.indices[p] : 0, 0}; },
            [&](int s, int, GateTriple<VEC, NCHUNK>& st, int) {
                const float* pk = a.k + (int64_t)s * a.ldk;
                const float* pa = a.a + (int64_t)s * a.lda;
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c) {
                    vload<VEC>(st.k[c], pk + tile.off[c]);
                    vload<VEC>(st.a[c], pa + tile.off[c]);
                    if constexpr (NORM) vload<VEC>(st.b[c], a.b + (int64_t)s * a.ldb + tile.off[c]);
                }
            },
            [&](int, int, const GateTriple<VEC, NCHUNK>& st, int) {
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c)
#pragma unroll
                    for (int t = 0; t < VEC; ++t) {
                        const Gate g = gate_of(st.k[c][t] + qv[c][t]);
                        if (wq) {
                            const float m = NORM ? fmaf(vv[c][t], st.a[c][t], st.b[c][t]) : vv[c][t] * st.a[c][t];
                            dq[c][t] = fmaf(g.g * g.gbar, m, dq[c][t]);
                        }
                        if (wv) dv[c][t] = fmaf(g.g, st.a[c][t], dv[c][t]);
                    }
            });
        // a chunk of a long row: its partial dq in plane 0 and dv in the plane behind the ones that are there
        if (wq) tile.store(sum_row(it, a.o0, a.ld0, a.ws, a.F), dq);
        if (wv) tile.store(sum_row(it, a.o1, a.ld1, a.ws + (wq ? a.plane : 0), a.F), dv);
    }
}

enum GateKind { GATE_FWD, GATE_BWD_DST, GATE_BWD_SRC };

template <int KIND, bool NORM>
struct GateLaunch {
    const GateArgs& a;
    hipStream_t st;
    template <int VEC, int LANES, int NCHUNK>
    void run() const {
        const int64_t blocks = (a.n_items * LANES + kBlock - 1) / kBlock;
        if (blocks == 0) return;
        const dim3 grid((unsigned)blocks), block(kBlock);
        if constexpr (KIND == GATE_FWD) {
            set_kernel("bot::spmm_gate_kernel<%d,%d,%d,%d>", (int)NORM, VEC, LANES, NCHUNK);
            hipLaunchKernelGGL((spmm_gate_kernel<NORM, VEC, LANES, NCHUNK>), grid, block, 0, st, a);
        } else if constexpr (KIND == GATE_BWD_DST) {
            set_kernel("bot::spmm_gate_bwd_dst_kernel<%d,%d,%d,%d>", (int)NORM, VEC, LANES, NCHUNK);
            hipLaunchKernelGGL((spmm_gate_bwd_dst_kernel<NORM, VEC, LANES, NCHUNK>), grid, block, 0, st, a);
        } else {
            set_kernel("bot::spmm_gate_bwd_src_kernel<%d,%d,%d,%d>", (int)NORM, VEC, LANES, NCHUNK);
            hipLaunchKernelGGL((spmm_gate_bwd_src_kernel<NORM, VEC, LANES, NCHUNK>), grid, block, 0, st, a);
        }
    }
    template <int VEC>
    void wide(int) const {
        // two staged rows per neighbour in the sweeps over destinations: tiles of 128 lanes; three over the sources: tiles of 64 lanes
        // keep the registers of four neighbours in flight
        if constexpr (KIND == GATE_BWD_SRC) run<VEC, 64, 1>();
        else run<VEC, 64, 2>();
    }
};

template <int KIND>
static void gate_dispatch(const GateArgs& a, bool norm, int vec, hipStream_t st) {
    if (norm) dispatch_sweep(GateLaunch<KIND, true>{a, st}, a.F, vec);
    else dispatch_sweep(GateLaunch<KIND, false>{a, st}, a.F, vec);
}

}  // namespace bot

extern "C" {

#define GATE_COMMON(name)                                                                                \
    if (int rc = check_plan_sizes(name, n_rows, nnz, n_items, n_long, n_slots)) return rc;              \
    BOT_REQUIRE(F >= 1, BOT_E_RANGE, name ": F=%d (>= 1)", F);

int bot_spmm_gate_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                      const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots, const float* k, int64_t ldk,
                      const float* q, int64_t ldq, const float* v, int64_t ldv, int32_t F, int32_t normalize, float eps, float* out, int64_t ldo,
                      float* den, int64_t ldden, void* workspace, bot_stream_t stream) {
    using namespace bot;
    (void)indptr;
    GATE_COMMON("spmm_gate")
    BOT_REQUIRE(std::isfinite(eps) && eps >= 0.f, BOT_E_RANGE, "spmm_gate: eps must be finite and not negative");
    if (n_rows == 0) return 0;
    const bool norm = normalize != 0;
    if (int rc = check_plan("spmm_gate", items, norm ? "items/k/out/den" : "items/k/out", k && out && (!norm || den), nnz, "indices/q/v",
                            indices && q && v, n_long, "long_rows/long_ptr/workspace", long_rows && long_ptr && workspace))
        return rc;
    if (!norm) den = nullptr;  // neither computed nor stored
    BOT_REQUIRE(n_long == 0 || n_slots > 0, BOT_E_RANGE, "spmm_gate: long rows without slots");
    BOT_REQUIRE(out != k && out != q && out != v && den != k && den != q && den != v && out != den, BOT_E_RANGE,
                "spmm_gate: out and den alias an input or each other");
    BOT_REQUIRE(ldk >= F && ldo >= F && (nnz == 0 || (ldq >= F && ldv >= F)) && (!den || ldden >= F), BOT_E_RANGE,
                "spmm_gate: row strides smaller than F=%d (ldk=%lld ldq=%lld ldv=%lld ldo=%lld ldden=%lld)", F, (long long)ldk, (long long)ldq,
                (long long)ldv, (long long)ldo, (long long)ldden);
    BOT_REQUIRE(aligned(k, 4) && aligned(q, 4) && aligned(v, 4) && aligned(out, 4) && aligned(den, 4) && aligned(items, 16) &&
                    aligned(workspace, 16),
                BOT_E_ALIGN, "spmm_gate: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    const GateArgs a{indices, reinterpret_cast<const int4*>(items), n_items, k, ldk, q, ldq, v, ldv, nullptr, 0, nullptr, 0, F, eps, out, ldo,
                     den, den ? ldden : F, static_cast<float*>(workspace), n_slots * F};
    // (the workspace: 16-byte base, planes of n_slots * F floats, slot rows of F floats - F % vec == 0 keeps every row aligned)
    const int vec = pick_vec(F, {ldk, ldq, ldv, ldo, a.ld1}, {k, q, v, out, den});
    gate_dispatch<GATE_FWD>(a, norm, vec, st);
    if (int rc = hip_status("spmm_gate launch")) return rc;
    if (n_long > 0) {
        if (norm)
            hipLaunchKernelGGL(spmm_gate_combine_kernel, dim3((unsigned)((n_long * F + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, a, long_rows,
                               long_ptr, n_long);
        else launch_sum_combine(a.ws, F, out, ldo, long_rows, long_ptr, n_long, st);
        if (int rc = hip_status("spmm_gate combine launch")) return rc;
    }
    return 0;
}

int bot_spmm_gate_bwd_dst_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items,
                              int64_t n_items, const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, const float* k, int64_t ldk,
                              const float* q, int64_t ldq, const float* v, int64_t ldv, const float* a, int64_t lda, const float* b, int64_t ldb,
                              int32_t F, float* dk, int64_t lddk, float* partial, bot_stream_t stream) {
    using namespace bot;
    (void)indptr;
    const int64_t n_slots = 0;
    GATE_COMMON("spmm_gate_bwd_dst")
    if (n_rows == 0) return 0;
    if (int rc = check_plan("spmm_gate_bwd_dst", items, "items/k/a/dk", k && a && dk, nnz, "indices/q/v", indices && q && v, n_long,
                            "long_rows/long_ptr/partial", long_rows && long_ptr && partial))
        return rc;
    BOT_REQUIRE(dk != k && dk != q && dk != v && dk != a && dk != b, BOT_E_RANGE, "spmm_gate_bwd_dst: dk aliases an input");
    BOT_REQUIRE(ldk >= F && lda >= F && lddk >= F && (!b || ldb >= F) && (nnz == 0 || (ldq >= F && ldv >= F)), BOT_E_RANGE,
                "spmm_gate_bwd_dst: row strides smaller than F=%d (ldk=%lld ldq=%lld ldv=%lld lda=%lld ldb=%lld lddk=%lld)", F, (long long)ldk,
                (long long)ldq, (long long)ldv, (long long)lda, (long long)ldb, (long long)lddk);
    BOT_REQUIRE(aligned(k, 4) && aligned(q, 4) && aligned(v, 4) && aligned(a, 4) && aligned(b, 4) && aligned(dk, 4) && aligned(items, 16) &&
                    aligned(partial, 16),
                BOT_E_ALIGN, "spmm_gate_bwd_dst: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    const GateArgs g{indices, reinterpret_cast<const int4*>(items), n_items, k, ldk, q, ldq, v, ldv, a, lda, b, b ? ldb : F, F, 0.f, dk, lddk,
                     nullptr, F, partial, 0};
    const int vec = pick_vec(F, {ldk, ldq, ldv, lda, g.ldb, lddk}, {k, q, v, a, b, dk});
    gate_dispatch<GATE_BWD_DST>(g, b != nullptr, vec, st);
    if (int rc = hip_status("spmm_gate_bwd_dst launch")) return rc;
    if (n_long > 0) {
        launch_sum_combine(partial, F, dk, lddk, long_rows, long_ptr, n_long, st);
        if (int rc = hip_status("spmm_gate_bwd_dst combine launch")) return rc;
    }
    return 0;
}

int bot_spmm_gate_bwd_src_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items,
                              int64_t n_items, const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots, const float* k,
                              int64_t ldk, const float* q, int64_t ldq, const float* v, int64_t ldv, const float* a, int64_t lda, const float* b,
                              int64_t ldb, int32_t F, float* dq, int64_t lddq, float* dv, int64_t lddv, float* partial, bot_stream_t stream) {
    using namespace bot;
    (void)indptr;
    GATE_COMMON("spmm_gate_bwd_src")
    if (n_rows == 0 || (!dq && !dv)) return 0;
    if (int rc = check_plan("spmm_gate_bwd_src", items, "items/q/v", q && v, nnz, "indices/k/a", indices && k && a, n_long,
                            "long_rows/long_ptr/partial", long_rows && long_ptr && partial))
        return rc;
    BOT_REQUIRE(n_long == 0 || n_slots > 0, BOT_E_RANGE, "spmm_gate_bwd_src: long rows without slots");
    BOT_REQUIRE((!dq || (dq != k && dq != q && dq != v && dq != a && dq != b)) && (!dv || (dv != k && dv != q && dv != v && dv != a && dv != b)) &&
                    (!dq || dq != dv),
                BOT_E_RANGE, "spmm_gate_bwd_src: dq and dv alias an input or each other");
    BOT_REQUIRE(ldq >= F && ldv >= F && (!dq || lddq >= F) && (!dv || lddv >= F) && (nnz == 0 || (ldk >= F && lda >= F && (!b || ldb >= F))),
                BOT_E_RANGE, "spmm_gate_bwd_src: row strides smaller than F=%d (ldk=%lld ldq=%lld ldv=%lld lda=%lld ldb=%lld lddq=%lld lddv=%lld)", F,
                (long long)ldk, (long long)ldq, (long long)ldv, (long long)lda, (long long)ldb, (long long)lddq, (long long)lddv);
    BOT_REQUIRE(aligned(k, 4) && aligned(q, 4) && aligned(v, 4) && aligned(a, 4) && aligned(b, 4) && aligned(dq, 4) && aligned(dv, 4) &&
                    aligned(items, 16) && aligned(partial, 16),
                BOT_E_ALIGN, "spmm_gate_bwd_src: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    const GateArgs g{indices, reinterpret_cast<const int4*>(items), n_items, k, ldk, q, ldq, v, ldv, a, lda, b, b ? ldb : F, F, 0.f, dq,
                     dq ? lddq : F, dv, dv ? lddv : F, partial, n_slots * F};
    const int vec = pick_vec(F, {ldk, ldq, ldv, lda, g.ldb, g.ld0, g.ld1}, {k, q, v, a, b, dq, dv});
    gate_dispatch<GATE_BWD_SRC>(g, b != nullptr, vec, st);
    if (int rc = hip_status("spmm_gate_bwd_src launch")) return rc;
    if (n_long > 0) {
        if (dq) launch_sum_combine(partial, F, dq, lddq, long_rows, long_ptr, n_long, st);
        if (dv) launch_sum_combine(partial + (dq ? g.plane : 0), F, dv, lddv, long_rows, long_ptr, n_long, st);
        if (int rc = hip_status("spmm_gate_bwd_src combine launch")) return rc;
    }
    return 0;
}

}  // extern "C"
