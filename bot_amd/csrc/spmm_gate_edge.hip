// Gated aggregation with an edge stream (include/bot_gnn.h "Gated aggregation with an edge stream") for gfx950: the GatedGCN layer of
// Bresson & Laurent, "Residual Gated Graph ConvNets" (arXiv:1711.07553) as Dwivedi et al., "Benchmarking Graph Neural Networks"
// (arXiv:2003.00982) and GraphGPS run it, DGL's GatedGCNConv; bot_amd.nn.GatedGCNConv, `ops.gated_edge_sum`.  The gate's pre-activation
// has a per-EDGE term and is itself the layer's second output, so [E, F] is the model's state here: these sweeps touch it exactly as
// often as the model forces and materialise nothing else per edge.  With j a position of the CSC, u its source, w its destination:
//   forward        s_j = (k[w] + q[u]) + c[j]  (two rounded additions),  e[j] = s_j  (stored unless e is NULL),  g_j = gate_of(s_j).g
//                  num[w] = sum_j g_j v[u],  den[w] = sum_j g_j;  out = num, or - normalised - num / (den + eps)     (rows = destinations)
//   backward, CSC  g_j, g'_j from the stored e[j];  ds[j] = de[j] + g'_j (v[u] a[w] + b[w])  (de NULL: zero);  dk[w] = sum_j ds[j]
//                  ds is the gradient of c and the operand of the source side                                        (rows = destinations)
//   backward, CSR  dq[u] = sum_j ds[pos_j],  dv[u] = sum_j gate_of(e[pos_j]).g a[w_j]         (rows = sources; pos = csr2csc, w_j = indices)
// with a = dout (b absent), or - normalised - a = dout / (den + eps), b = -a out, formed by the caller with dense ops.
//
// The gather is the lane-group row sweep of sweep.h (walk_row), lane layout as in bot_spmm_gate_f32, the gate is gate.h's gate_of.  The
// row a group owns (k of the destination; a and b in the backward) stays in registers across its neighbours.  c, e, de and ds are
// STREAMED rows: read or written at the walk's own position, one contiguous row per step, never gathered (the CSR sweep reaches them
// through pos: there they are gathers).  e may alias c and ds may alias de: each element is read and then written by the same lane.
// The sums run in position order in registers; the chunks of a long row store the per-edge rows of their OWN positions and leave their
// partial sums in the workspace, folded in slot order (the normalised forward divides after the fold).  Every product is rounded on its
// own and every fused multiply-add is written out (smx.h switches contraction off).  No atomics: the bytes repeat from call to call.
// `stream_nt` != 0 marks the accesses to the streamed rows non-temporal (the A/B of README "GatedGCN with an edge stream"); values and
// bytes are the same either way.
//
// HBM model (4-byte words; derived, not measured):
//   forward        4 [E (1 + 2F + 2F) + n_dst F (2 or 3)]         ids, the (q, v) pair gathered, c read and e written per edge; k read,
//                                                                  out (and den) written per row
//   backward, CSC  4 [E (1 + F + F + F + F) + n_dst F (3 or 4)]   ids, v gathered, e and de read, ds written per edge (less E F where de is
//                                                                  NULL); a (and b) read, dk written per row.  (This count keeps a row
//                                                                  term for k, as the gate sweeps' does; the gate comes from the stored
//                                                                  e, so k is not read and the sweep moves n_dst F words fewer: 2 or 3.)
//   backward, CSR  4 [E (2 + 3F) + 3 n_src F]                     ids and positions, ds, e and a per out-edge; dq and dv written per row
#include "sweep.h"

#include <cmath>
#include <initializer_list>

// (contraction off for the rest of this file: see above)
#include "gate.h"

namespace bot {

struct GateEdgeArgs {
    const int32_t* indices;
    const int32_t* pos;  // CSR sweep: the CSC position of every out-edge
    const int4* items;
    int64_t n_items;
    const float* k;  // forward: [n_dst, F]
    int64_t ldk;
    const float* q;  // forward: [n_src, F]
    int64_t ldq;
    const float* v;  // forward, backward CSC: [n_src, F]
    int64_t ldv;
    const float* a;  // backward: [n_dst, F]
    int64_t lda;
    const float* b;  // backward CSC, normalised: [n_dst, F]
    int64_t ldb;
    const float* c;  // forward: [E, F] in position order; backward: the stored e
    int64_t ldc;
    float* e;  // forward: e out (NULL: not stored); backward CSC: ds out (NULL: not stored)
    int64_t lde;
    const float* de;  // backward CSC: upstream gradient of e (NULL: zero); backward CSR: ds
    int64_t ldde;
    int32_t F;
    int32_t nt;
    float eps;
    float* o0;  // forward: out; backward CSC: dk (NULL: not asked for); backward CSR: dq (NULL: not asked for)
    int64_t ld0;
    float* o1;  // forward: den (normalised); backward CSR: dv (NULL: not asked for)
    int64_t ld1;
    float* ws;      // the long rows' chunks: planes of n_slots * F floats
    int64_t plane;  // n_slots * F
};

// A streamed row's accesses: ordinary, or marked non-temporal
template <int VEC>
__device__ __forceinline__ void sload(float (&r)[VEC], const float* p, bool nt) {
    if (nt) {
        typedef float nv __attribute__((ext_vector_type(VEC)));
        const nv x = __builtin_nontemporal_load(reinterpret_cast<const nv*>(p));
#pragma unroll
        for (int t = 0; t < VEC; ++t) r[t] = x[t];
    } else {
        vload<VEC>(r, p);
    }
}
template <int VEC>
__device__ __forceinline__ void sstore(float* p, const float (&r)[VEC], bool nt) {
    if (nt) vstore_nt<VEC>(p, r);
    else vstore<VEC>(p, r);
}

template <int VEC, int NCHUNK>
struct GateEdgeStage {
    float x[NCHUNK][VEC], y[NCHUNK][VEC], z[NCHUNK][VEC];  // forward: q, v, c; backward CSC: v, e, de; backward CSR: ds, e, a
};

template <bool NORM, int VEC, int LANES, int NCHUNK>
__global__ __launch_bounds__(kBlock) void spmm_gate_edge_kernel(GateEdgeArgs a) {
    constexpr int TILE = LANES * VEC * NCHUNK;
    using Stage = GateEdgeStage<VEC, NCHUNK>;
    const int lane = threadIdx.x % LANES;
    const int64_t item = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / LANES;
    if (item >= a.n_items) return;  // whole groups leave together
    const RowItem it = load_item<LANES>(a.items, item);
    const bool nt = a.nt != 0, we = a.e != nullptr;  // uniform over the launch
    for (int col0 = 0; col0 < a.F; col0 += TILE) {  // groups narrower than a wavefront have one tile
        const ColTile<VEC, LANES, NCHUNK> tile(col0, lane, a.F);
        float kv[NCHUNK][VEC], num[NCHUNK][VEC] = {}, den[NCHUNK][VEC] = {};
#pragma unroll
        for (int c = 0; c < NCHUNK; ++c) vload<VEC>(kv[c], a.k + (int64_t)it.row * a.ldk + tile.off[c]);
        walk_row<LANES, Stage>(
            it.beg, it.end, lane, [&](int p, bool in) { return Edge{in ? a.indices[p] : 0, 0}; },
            [&](int s, int, Stage& st, int p) {
                const float* pq = a.q + (int64_t)s * a.ldq;
                const float* pv = a.v + (int64_t)s * a.ldv;
                const float* pc = a.c + (int64_t)p * a.ldc;
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c) {
                    vload<VEC>(st.x[c], pq + tile.off[c]);
                    vload<VEC>(st.y[c], pv + tile.off[c]);
                    sload<VEC>(st.z[c], pc + tile.off[c], nt);
                }
            },
            [&](int, int, const Stage& st, int p) {
                float* pe = a.e + (int64_t)p * a.lde;
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c) {
                    float sv[VEC];
#pragma unroll
                    for (int t = 0; t < VEC; ++t) {
                        sv[t] = (kv[c][t] + st.x[c][t]) + st.z[c][t];
                        const float g = gate_of(sv[t]).g;
                        num[c][t] = fmaf(g, st.y[c][t], num[c][t]);
                        if constexpr (NORM) den[c][t] += g;
                    }
                    if (we && tile.act[c]) sstore<VEC>(pe + tile.off[c], sv, nt);
                }
            });
        if (it.slot >= 0) {  // a chunk of a long row: the raw sums into the workspace (its e rows are stored above)
            float* w = a.ws + (int64_t)it.slot * a.F;
            tile.store(w, num);
            if constexpr (NORM) tile.store(w + a.plane, den);
            continue;
        }
        if constexpr (NORM) {
#pragma unroll
            for (int c = 0; c < NCHUNK; ++c)
#pragma unroll
                for (int t = 0; t < VEC; ++t) num[c][t] = num[c][t] / (den[c][t] + a.eps);
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
__global__ __launch_bounds__(kBlock) void spmm_gate_edge_combine_kernel(GateEdgeArgs a, const int32_t* long_rows, const int32_t* long_ptr,
                                                                        int64_t n_long) {
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

// Backward over the CSC: the row owner holds a (and b) of its destination; per position the source's v row and the streamed e, de, ds.
template <bool NORM, int VEC, int LANES, int NCHUNK>
__global__ __launch_bounds__(kBlock) void spmm_gate_edge_bwd_kernel(GateEdgeArgs a) {
    constexpr int TILE = LANES * VEC * NCHUNK;
    using Stage = GateEdgeStage<VEC, NCHUNK>;
    const int lane = threadIdx.x % LANES;
    const int64_t item = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / LANES;
    if (item >= a.n_items) return;  // whole groups leave together
    const RowItem it = load_item<LANES>(a.items, item);
    const bool nt = a.nt != 0, hd = a.de != nullptr, wds = a.e != nullptr, wk = a.o0 != nullptr;  // uniform over the launch
    for (int col0 = 0; col0 < a.F; col0 += TILE) {
        const ColTile<VEC, LANES, NCHUNK> tile(col0, lane, a.F);
        float av[NCHUNK][VEC], bv[NCHUNK][VEC] = {}, acc[NCHUNK][VEC] = {};
#pragma unroll
        for (int c = 0; c < NCHUNK; ++c) {
            vload<VEC>(av[c], a.a + (int64_t)it.row * a.lda + tile.off[c]);
            if constexpr (NORM) vload<VEC>(bv[c], a.b + (int64_t)it.row * a.ldb + tile.off[c]);
        }
        walk_row<LANES, Stage>(
            it.beg, it.end, lane, [&](int p, bool in) { return Edge{in ? a.indices[p] : 0, 0}; },
            [&](int s, int, Stage& st, int p) {
                const float* pv = a.v + (int64_t)s * a.ldv;
                const float* pe = a.c + (int64_t)p * a.ldc;
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c) {
                    vload<VEC>(st.x[c], pv + tile.off[c]);
                    sload<VEC>(st.y[c], pe + tile.off[c], nt);
                    if (hd) sload<VEC>(st.z[c], a.de + (int64_t)p * a.ldde + tile.off[c], nt);
                }
            },
            [&](int, int, const Stage& st, int p) {
                float* pds = a.e + (int64_t)p * a.lde;
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c) {
                    float dsv[VEC];
#pragma unroll
                    for (int t = 0; t < VEC; ++t) {
                        const Gate g = gate_of(st.y[c][t]);
                        const float m = NORM ? fmaf(st.x[c][t], av[c][t], bv[c][t]) : st.x[c][t] * av[c][t];
                        const float term = (g.g * g.gbar) * m;
                        dsv[t] = hd ? st.z[c][t] + term : term;
                        acc[c][t] += dsv[t];
                    }
                    if (wds && tile.act[c]) sstore<VEC>(pds + tile.off[c], dsv, nt);
                }
            });
        if (wk) tile.store(sum_row(it, a.o0, a.ld0, a.ws, a.F), acc);
    }
}

// Backward over the CSR: per out-edge the rows of ds and e at its CSC position and a of its destination; nothing is held across the row.
template <int VEC, int LANES, int NCHUNK>
__global__ __launch_bounds__(kBlock) void spmm_gate_edge_bwd_src_kernel(GateEdgeArgs a) {
    constexpr int TILE = LANES * VEC * NCHUNK;
    using Stage = GateEdgeStage<VEC, NCHUNK>;
    const int lane = threadIdx.x % LANES;
    const int64_t item = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / LANES;
    if (item >= a.n_items) return;  // whole groups leave together
    const RowItem it = load_item<LANES>(a.items, item);
    const bool wq = a.o0 != nullptr, wv = a.o1 != nullptr;  // uniform over the launch
    for (int col0 = 0; col0 < a.F; col0 += TILE) {
        const ColTile<VEC, LANES, NCHUNK> tile(col0, lane, a.F);
        float dq[NCHUNK][VEC] = {}, dv[NCHUNK][VEC] = {};
        walk_row<LANES, Stage>(
            it.beg, it.end, lane, [&](int p, bool in) { return in ? Edge{a.indices[p], a.pos[p]} : Edge{0, 0}; },
            [&](int w, int j, Stage& st, int) {
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c) {
                    if (wq) vload<VEC>(st.x[c], a.de + (int64_t)j * a.ldde + tile.off[c]);
                    if (wv) {
                        vload<VEC>(st.y[c], a.c + (int64_t)j * a.ldc + tile.off[c]);
                        vload<VEC>(st.z[c], a.a + (int64_t)w * a.lda + tile.off[c]);
                    }
                }
            },
            [&](int, int, const Stage& st, int) {
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c)
#pragma unroll
                    for (int t = 0; t < VEC; ++t) {
                        if (wq) dq[c][t] += st.x[c][t];
                        if (wv) dv[c][t] = fmaf(gate_of(st.y[c][t]).g, st.z[c][t], dv[c][t]);
                    }
            });
        // a chunk of a long row: its partial dq in plane 0 and dv in the plane behind the ones that are there
        if (wq) tile.store(sum_row(it, a.o0, a.ld0, a.ws, a.F), dq);
        if (wv) tile.store(sum_row(it, a.o1, a.ld1, a.ws + (wq ? a.plane : 0), a.F), dv);
    }
}

enum GateEdgeKind { GATE_EDGE_FWD, GATE_EDGE_BWD, GATE_EDGE_BWD_SRC };

template <int KIND, bool NORM>
struct GateEdgeLaunch {
    const GateEdgeArgs& a;
    hipStream_t st;
    template <int VEC, int LANES, int NCHUNK>
    void run() const {
        const int64_t blocks = (a.n_items * LANES + kBlock - 1) / kBlock;
        if (blocks == 0) return;
        const dim3 grid((unsigned)blocks), block(kBlock);
        if constexpr (KIND == GATE_EDGE_FWD) {
            set_kernel("bot::spmm_gate_edge_kernel<%d,%d,%d,%d>", (int)NORM, VEC, LANES, NCHUNK);
            hipLaunchKernelGGL((spmm_gate_edge_kernel<NORM, VEC, LANES, NCHUNK>), grid, block, 0, st, a);
        } else if constexpr (KIND == GATE_EDGE_BWD) {
            set_kernel("bot::spmm_gate_edge_bwd_kernel<%d,%d,%d,%d>", (int)NORM, VEC, LANES, NCHUNK);
            hipLaunchKernelGGL((spmm_gate_edge_bwd_kernel<NORM, VEC, LANES, NCHUNK>), grid, block, 0, st, a);
        } else {
            set_kernel("bot::spmm_gate_edge_bwd_src_kernel<%d,%d,%d>", VEC, LANES, NCHUNK);
            hipLaunchKernelGGL((spmm_gate_edge_bwd_src_kernel<VEC, LANES, NCHUNK>), grid, block, 0, st, a);
        }
    }
    template <int VEC>
    void wide(int) const {
        run<VEC, 64, 1>();  // three staged rows per position: tiles of 64 lanes keep the registers of four positions in flight
    }
};

template <int KIND>
static void gate_edge_dispatch(const GateEdgeArgs& a, bool norm, int vec, hipStream_t st) {
    if (norm) dispatch_sweep(GateEdgeLaunch<KIND, true>{a, st}, a.F, vec);
    else dispatch_sweep(GateEdgeLaunch<KIND, false>{a, st}, a.F, vec);
}

}  // namespace bot

extern "C" {

#define GATE_EDGE_COMMON(name)                                                                           \
    if (int rc = check_plan_sizes(name, n_rows, nnz, n_items, n_long, n_slots)) return rc;              \
    BOT_REQUIRE(F >= 1, BOT_E_RANGE, name ": F=%d (>= 1)", F);

int bot_spmm_gate_edge_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                           const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots, const float* k, int64_t ldk,
                           const float* q, int64_t ldq, const float* v, int64_t ldv, const float* c, int64_t ldc, int32_t F, int32_t normalize,
                           float eps, float* out, int64_t ldo, float* den, int64_t ldden, float* e, int64_t lde, int32_t stream_nt,
                           void* workspace, bot_stream_t stream) {
    using namespace bot;
    (void)indptr;
    GATE_EDGE_COMMON("spmm_gate_edge")
    BOT_REQUIRE(std::isfinite(eps) && eps >= 0.f, BOT_E_RANGE, "spmm_gate_edge: eps must be finite and not negative");
    if (n_rows == 0) return 0;
    const bool norm = normalize != 0;
    if (int rc = check_plan("spmm_gate_edge", items, norm ? "items/k/out/den" : "items/k/out", k && out && (!norm || den), nnz, "indices/q/v/c",
                            indices && q && v && c, n_long, "long_rows/long_ptr/workspace", long_rows && long_ptr && workspace))
        return rc;
    if (!norm) den = nullptr;  // neither computed nor stored
    BOT_REQUIRE(n_long == 0 || n_slots > 0, BOT_E_RANGE, "spmm_gate_edge: long rows without slots");
    BOT_REQUIRE(out != k && out != q && out != v && out != c && den != k && den != q && den != v && den != c && out != den &&
                    (!e || (e != k && e != q && e != v && e != out && e != den)) && (e != c || lde == ldc),
                BOT_E_RANGE, "spmm_gate_edge: out, den and e alias an input or each other (e may be c itself, with c's pitch)");
    BOT_REQUIRE(ldk >= F && ldo >= F && (nnz == 0 || (ldq >= F && ldv >= F && ldc >= F && (!e || lde >= F))) && (!den || ldden >= F),
                BOT_E_RANGE, "spmm_gate_edge: row strides smaller than F=%d (ldk=%lld ldq=%lld ldv=%lld ldc=%lld ldo=%lld ldden=%lld lde=%lld)", F,
                (long long)ldk, (long long)ldq, (long long)ldv, (long long)ldc, (long long)ldo, (long long)ldden, (long long)lde);
    BOT_REQUIRE(aligned(k, 4) && aligned(q, 4) && aligned(v, 4) && aligned(c, 4) && aligned(e, 4) && aligned(out, 4) && aligned(den, 4) &&
                    aligned(items, 16) && aligned(workspace, 16),
                BOT_E_ALIGN, "spmm_gate_edge: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    GateEdgeArgs a{};
    a.indices = indices, a.items = reinterpret_cast<const int4*>(items), a.n_items = n_items;
    a.k = k, a.ldk = ldk, a.q = q, a.ldq = ldq, a.v = v, a.ldv = ldv, a.c = c, a.ldc = ldc, a.e = e, a.lde = e ? lde : F;
    a.F = F, a.nt = stream_nt, a.eps = eps, a.o0 = out, a.ld0 = ldo, a.o1 = den, a.ld1 = den ? ldden : F;
    a.ws = static_cast<float*>(workspace), a.plane = n_slots * F;
    const int vec = pick_vec(F, {ldk, ldq, ldv, ldc, a.lde, ldo, a.ld1}, {k, q, v, c, e, out, den});
    gate_edge_dispatch<GATE_EDGE_FWD>(a, norm, vec, st);
    if (int rc = hip_status("spmm_gate_edge launch")) return rc;
    if (n_long > 0) {
        if (norm)
            hipLaunchKernelGGL(spmm_gate_edge_combine_kernel, dim3((unsigned)((n_long * F + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, a,
                               long_rows, long_ptr, n_long);
        else launch_sum_combine(a.ws, F, out, ldo, long_rows, long_ptr, n_long, st);
        if (int rc = hip_status("spmm_gate_edge combine launch")) return rc;
    }
    return 0;
}

int bot_spmm_gate_edge_bwd_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items,
                               int64_t n_items, const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, const float* v, int64_t ldv,
                               const float* e, int64_t lde, const float* a, int64_t lda, const float* b, int64_t ldb, const float* de,
                               int64_t ldde, int32_t F, float* ds, int64_t ldds, float* dk, int64_t lddk, int32_t stream_nt, float* partial,
                               bot_stream_t stream) {
    using namespace bot;
    (void)indptr;
    const int64_t n_slots = 0;
    GATE_EDGE_COMMON("spmm_gate_edge_bwd")
    if (n_rows == 0 || (!ds && !dk)) return 0;
    if (int rc = check_plan("spmm_gate_edge_bwd", items, "items/a", a != nullptr, nnz, "indices/v/e", indices && v && e, dk ? n_long : 0,
                            "long_rows/long_ptr/partial", long_rows && long_ptr && partial))
        return rc;
    BOT_REQUIRE((!dk || (dk != v && dk != e && dk != a && dk != b && dk != de && dk != ds)) &&
                    (!ds || (ds != v && ds != e && ds != a && ds != b)) && (!ds || ds != de || ldds == ldde),
                BOT_E_RANGE, "spmm_gate_edge_bwd: ds and dk alias an input or each other (ds may be de itself, with de's pitch)");
    BOT_REQUIRE(lda >= F && (!dk || lddk >= F) && (!b || ldb >= F) &&
                    (nnz == 0 || (ldv >= F && lde >= F && (!de || ldde >= F) && (!ds || ldds >= F))),
                BOT_E_RANGE, "spmm_gate_edge_bwd: row strides smaller than F=%d (ldv=%lld lde=%lld lda=%lld ldb=%lld ldde=%lld ldds=%lld lddk=%lld)",
                F, (long long)ldv, (long long)lde, (long long)lda, (long long)ldb, (long long)ldde, (long long)ldds, (long long)lddk);
    BOT_REQUIRE(aligned(v, 4) && aligned(e, 4) && aligned(a, 4) && aligned(b, 4) && aligned(de, 4) && aligned(ds, 4) && aligned(dk, 4) &&
                    aligned(items, 16) && aligned(partial, 16),
                BOT_E_ALIGN, "spmm_gate_edge_bwd: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    GateEdgeArgs g{};
    g.indices = indices, g.items = reinterpret_cast<const int4*>(items), g.n_items = n_items;
    g.v = v, g.ldv = ldv, g.c = e, g.ldc = lde, g.a = a, g.lda = lda, g.b = b, g.ldb = b ? ldb : F, g.de = de, g.ldde = de ? ldde : F;
    g.e = ds, g.lde = ds ? ldds : F, g.F = F, g.nt = stream_nt, g.o0 = dk, g.ld0 = dk ? lddk : F, g.ws = partial;
    const int vec = pick_vec(F, {ldv, lde, lda, g.ldb, g.ldde, g.lde, g.ld0}, {v, e, a, b, de, ds, dk});
    gate_edge_dispatch<GATE_EDGE_BWD>(g, b != nullptr, vec, st);
    if (int rc = hip_status("spmm_gate_edge_bwd launch")) return rc;
    if (n_long > 0 && dk) {
        launch_sum_combine(partial, F, dk, lddk, long_rows, long_ptr, n_long, st);
        if (int rc = hip_status("spmm_gate_edge_bwd combine launch")) return rc;
    }
    return 0;
}

int bot_spmm_gate_edge_bwd_src_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items,
                                   int64_t n_items, const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots,
                                   const int32_t* pos, const float* e, int64_t lde, const float* ds, int64_t ldds, const float* a, int64_t lda,
                                   int32_t F, float* dq, int64_t lddq, float* dv, int64_t lddv, float* partial, bot_stream_t stream) {
    using namespace bot;
    (void)indptr;
    GATE_EDGE_COMMON("spmm_gate_edge_bwd_src")
    if (n_rows == 0 || (!dq && !dv)) return 0;
    if (int rc = check_plan("spmm_gate_edge_bwd_src", items, "items", true, nnz, "indices/pos/ds (for dq)/e/a (for dv)",
                            indices && pos && (!dq || ds) && (!dv || (e && a)), n_long, "long_rows/long_ptr/partial",
                            long_rows && long_ptr && partial))
        return rc;
    BOT_REQUIRE(n_long == 0 || n_slots > 0, BOT_E_RANGE, "spmm_gate_edge_bwd_src: long rows without slots");
    BOT_REQUIRE((!dq || (dq != e && dq != ds && dq != a)) && (!dv || (dv != e && dv != ds && dv != a)) && (!dq || dq != dv), BOT_E_RANGE,
                "spmm_gate_edge_bwd_src: dq and dv alias an input or each other");
    BOT_REQUIRE((!dq || lddq >= F) && (!dv || lddv >= F) && (nnz == 0 || ((!dq || ldds >= F) && (!dv || (lde >= F && lda >= F)))), BOT_E_RANGE,
                "spmm_gate_edge_bwd_src: row strides smaller than F=%d (lde=%lld ldds=%lld lda=%lld lddq=%lld lddv=%lld)", F, (long long)lde,
                (long long)ldds, (long long)lda, (long long)lddq, (long long)lddv);
    BOT_REQUIRE(aligned(e, 4) && aligned(ds, 4) && aligned(a, 4) && aligned(dq, 4) && aligned(dv, 4) && aligned(pos, 4) && aligned(items, 16) &&
                    aligned(partial, 16),
                BOT_E_ALIGN, "spmm_gate_edge_bwd_src: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    GateEdgeArgs g{};
    g.indices = indices, g.pos = pos, g.items = reinterpret_cast<const int4*>(items), g.n_items = n_items;
    if (dq) g.de = ds, g.ldde = ldds;
    else g.ldde = F;
    if (dv) g.c = e, g.ldc = lde, g.a = a, g.lda = lda;
    else g.ldc = g.lda = F;
    g.F = F, g.o0 = dq, g.ld0 = dq ? lddq : F, g.o1 = dv, g.ld1 = dv ? lddv : F, g.ws = partial, g.plane = n_slots * F;
    const int vec = pick_vec(F, {g.ldde, g.ldc, g.lda, g.ld0, g.ld1}, {g.de, g.c, g.a, dq, dv});
    gate_edge_dispatch<GATE_EDGE_BWD_SRC>(g, false, vec, st);
    if (int rc = hip_status("spmm_gate_edge_bwd_src launch")) return rc;
    if (n_long > 0) {
        if (dq) launch_sum_combine(partial, F, dq, lddq, long_rows, long_ptr, n_long, st);
        if (dv) launch_sum_combine(partial + (dq ? g.plane : 0), F, dv, lddv, long_rows, long_ptr, n_long, st);
        if (int rc = hip_status("spmm_gate_edge_bwd_src combine launch")) return rc;
    }
    return 0;
}

}  // extern "C"
