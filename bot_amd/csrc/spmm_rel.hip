// Relation sweeps (include/bot_gnn.h "Relational aggregation") for gfx950: the aggregation of the relational GCN of Schlichtkrull et
// al., "Modeling Relational Data with Graph Convolutional Networks" (ESWC 2018; DGL's RelGraphConv, PyG's RGCNConv) with the basis
// regulariser W_r = sum_b coef[r,b] V_b; bot_amd.nn.RelGraphConv, `ops.rel_expand_sum` / `ops.rel_contract_sum`.  Position j of a row has a
// neighbour u_j, a relation r_j (etype[j]) and a constant weight c_j (norm[j], 1 without norm):
//   expand    Z[v,b,:]  = sum_j c_j coef[r_j,b] x[u_j,:]                 x [n_src, F]    -> Z   [n_rows, B, F]   one row gathered per edge
//   contract  out[v,:]  = sum_j c_j sum_b coef[r_j,b] y[u_j,b,:]         y [n_src, B, F] -> out [n_rows, F]      B column blocks per edge
// coef NULL is the one-hot mode, B = R and coef the identity: expand adds c_j x[u_j] into accumulator r_j alone, contract gathers block
// r_j of the neighbour's row alone (F floats per edge, not R F).  The two are each other's transpose: the gradient of expand over the CSC
// is contract over the CSR applied to dZ, and the other way round, so these two kernels are the layer's forward and backward in both
// GEMM orders (aggregate-first: expand, then [n, B F_in] x [B F_in, F_out]; project-first: x [V_1 | ... | V_B], then contract).
//
// The gather is the lane-group row sweep that sweep.h describes (walk_row); the relation travels as the Edge word beside the id.  What is
// read per POSITION beside the neighbour's row - c_j and the coefficient row of r_j - is loaded in `fetch` into the staging slot by every
// lane of the group from ONE address (a broadcast load: one request per group, a scalar load where the group is a wavefront), so it is in
// flight with the row loads.  The table is R B floats and stays in the caches; no LDS, no second path.
//
// Arithmetic, the same for whole rows, chunks and the combine (contraction is off for this file, every fused multiply-add is written out):
//   expand    w = c_j * coef[r_j,b] (one rounding), acc_b = fma(w, x, acc_b) in position order; one-hot: acc_{r_j} = fma(c_j, x, acc_{r_j}).
//             At most 16 accumulator blocks are live: B > 16 walks the row again for every further 16 blocks of coefficient columns.
//   contract  t = coef[r_j,b0] y_b0, t = fma(coef[r_j,b], y_b, t) over the blocks of a pass in order, acc = fma(c_j, t, acc); one-hot:
//             acc = fma(c_j, y_{r_j}, acc).  B > 16 walks the row again per 16 blocks, on the same accumulator (pass-major order).
// norm NULL runs with c_j = 1.0f, so it gives the bytes of a norm of ones.  The chunks of a long row leave their sums in the workspace
// ([n_slots, B F] / [n_slots, F]) and launch_sum_combine folds them in slot order.  No atomics: the bytes repeat from call to call.
// Roundings per output entry of a row of n positions in m chunks: expand <= n + m, contract <= n P + m + min(B, 16), P = ceil(B / 16).
//
// HBM model (4-byte words; the coefficient table is not counted), for the comparison with the sum sweep (bot_spmm_f32) at the gathered width:
//   expand              4 [E (2 + [norm] + F) + n_rows B F]          ids, relations (and norm) and one x row per edge; Z written
//   contract            4 [E (2 + [norm] + B F) + n_rows F]          the B blocks of a y row per edge; out written
//   contract, one-hot   4 [E (2 + [norm] + F) + n_rows F]            one block per edge
#include "sweep.h"

#include <initializer_list>

// (contraction off for the rest of this file: see above)
#include "smx.h"

namespace bot {

struct RelArgs {
    const int32_t* indices;
    const int32_t* etype;  // [nnz], position order
    const float* norm;     // [nnz], position order, or NULL
    const float* coef;     // [R, B], or NULL: one-hot
    const int4* items;
    int64_t n_items;
    const float* x;  // expand: [n_src, F]; contract: [n_src, B, F]
    int64_t ldx;
    float* out;  // expand: [n_rows, B, F]; contract: [n_rows, F]
    int64_t ldo;
    float* ws;     // the long rows' chunks: [n_slots, B F] / [n_slots, F]
    int32_t F, B;  // B: coefficient columns (one-hot: R)
};

constexpr int kRelBlocks = 16;  // accumulator blocks (expand) / staged column blocks (contract) of one pass

template <int VEC, int NB>
struct ExpandStage {
    float x[VEC], w[NB];  // the neighbour's columns; c_j coef[r_j, b0 + b] (one-hot: w[0] = c_j)
};

template <int VEC, int NB>
struct ContractStage {
    float y[NB][VEC], w[NB], c;
};

// neighbours in flight per group: at most 16 staged blocks / 32 staged coefficients
constexpr int expand_unroll(int nb) { return nb >= 16 ? 2 : 4; }
constexpr int contract_unroll(int nb) { return nb >= 16 ? 1 : nb >= 8 ? 2 : 4; }

template <bool ONEHOT, int NB, int VEC, int LANES>
__global__ __launch_bounds__(kBlock) void spmm_rel_expand_kernel(RelArgs a) {
    constexpr int TILE = LANES * VEC;
    using Stage = ExpandStage<VEC, ONEHOT ? 1 : NB>;
    const int lane = threadIdx.x % LANES;
    const int64_t item = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / LANES;
    if (item >= a.n_items) return;  // whole groups leave together
    const RowItem it = load_item<LANES>(a.items, item);
    float* dst = it.slot >= 0 ? a.ws + (int64_t)it.slot * a.B * a.F : a.out + (int64_t)it.row * a.ldo;
    for (int b0 = 0; b0 < a.B; b0 += NB)                  // B <= 16: one pass
        for (int col0 = 0; col0 < a.F; col0 += TILE) {  // groups narrower than a wavefront have one tile
            const ColTile<VEC, LANES, 1> tile(col0, lane, a.F);
            float acc[NB][VEC] = {};
            walk_row<LANES, Stage, expand_unroll(NB)>(
                it.beg, it.end, lane, [&](int p, bool in) { return Edge{in ? a.indices[p] : 0, in ? a.etype[p] : 0}; },
                [&](int s, int r, Stage& st, int k) {
                    vload<VEC>(st.x, a.x + (int64_t)s * a.ldx + tile.off[0]);
                    const float c = a.norm ? a.norm[k] : 1.f;
                    if constexpr (ONEHOT) {
                        st.w[0] = c;
                    } else {
                        const float* cf = a.coef + (int64_t)r * a.B + b0;
#pragma unroll
                        for (int b = 0; b < NB; ++b) st.w[b] = b0 + b < a.B ? c * cf[b] : 0.f;
                    }
                },
                [&](int, int r, const Stage& st, int) {
#pragma unroll
                    for (int b = 0; b < NB; ++b)
#pragma unroll
                        for (int t = 0; t < VEC; ++t) {
                            if constexpr (ONEHOT) acc[b][t] = r == b0 + b ? fmaf(st.w[0], st.x[t], acc[b][t]) : acc[b][t];  // a select
                            else acc[b][t] = fmaf(st.w[b], st.x[t], acc[b][t]);
                        }
                });
            if (tile.act[0]) {
#pragma unroll
                for (int b = 0; b < NB; ++b)
                    if (b0 + b < a.B) vstore<VEC>(dst + (int64_t)(b0 + b) * a.F + tile.off[0], acc[b]);
            }
        }
}

template <bool ONEHOT, int NB, int VEC, int LANES>
__global__ __launch_bounds__(kBlock) void spmm_rel_contract_kernel(RelArgs a) {
    constexpr int TILE = LANES * VEC;
    using Stage = ContractStage<VEC, NB>;
    const int lane = threadIdx.x % LANES;
    const int64_t item = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / LANES;
    if (item >= a.n_items) return;  // whole groups leave together
    const RowItem it = load_item<LANES>(a.items, item);
    const int passes = ONEHOT ? 1 : (a.B + NB - 1) / NB;
    for (int col0 = 0; col0 < a.F; col0 += TILE) {
        const ColTile<VEC, LANES, 1> tile(col0, lane, a.F);
        float acc[VEC] = {};
        for (int p = 0; p < passes; ++p) {  // B <= 16: one pass
            const int b0 = p * NB;
            walk_row<LANES, Stage, contract_unroll(NB)>(
                it.beg, it.end, lane, [&](int q, bool in) { return Edge{in ? a.indices[q] : 0, in ? a.etype[q] : 0}; },
                [&](int s, int r, Stage& st, int k) {
                    const float* py = a.x + (int64_t)s * a.ldx + tile.off[0];
                    st.c = a.norm ? a.norm[k] : 1.f;
                    if constexpr (ONEHOT) {
                        vload<VEC>(st.y[0], py + (int64_t)r * a.F);
                    } else {
                        const float* cf = a.coef + (int64_t)r * a.B + b0;
#pragma unroll
                        for (int b = 0; b < NB; ++b) {
                            const bool in = b0 + b < a.B;
                            vload<VEC>(st.y[b], py + (int64_t)(in ? b0 + b : 0) * a.F);  // a block past B re-reads block 0 with weight 0
                            st.w[b] = in ? cf[b] : 0.f;
                        }
                    }
                },
                [&](int, int, const Stage& st, int) {
#pragma unroll
                    for (int t = 0; t < VEC; ++t) {
                        float m = st.y[0][t];
                        if constexpr (!ONEHOT) {
                            m = st.w[0] * m;
#pragma unroll
                            for (int b = 1; b < NB; ++b) m = fmaf(st.w[b], st.y[b][t], m);
                        }
                        acc[t] = fmaf(st.c, m, acc[t]);
                    }
                });
        }
        if (tile.act[0]) vstore<VEC>(sum_row(it, a.out, a.ldo, a.ws, a.F) + tile.off[0], acc);
    }
}

template <bool EXPAND, bool ONEHOT, int NB>
struct RelLaunch {
    const RelArgs& a;
    hipStream_t st;
    template <int VEC, int LANES, int NCHUNK>
    void run() const {
        const int64_t blocks = (a.n_items * LANES + kBlock - 1) / kBlock;
        if (blocks == 0) return;
        const dim3 grid((unsigned)blocks), block(kBlock);
        if constexpr (EXPAND) {
            set_kernel("bot::spmm_rel_expand_kernel<%d,%d,%d,%d>", (int)ONEHOT, NB, VEC, LANES);
            hipLaunchKernelGGL((spmm_rel_expand_kernel<ONEHOT, NB, VEC, LANES>), grid, block, 0, st, a);
        } else {
            set_kernel("bot::spmm_rel_contract_kernel<%d,%d,%d,%d>", (int)ONEHOT, NB, VEC, LANES);
            hipLaunchKernelGGL((spmm_rel_contract_kernel<ONEHOT, NB, VEC, LANES>), grid, block, 0, st, a);
        }
    }
    template <int VEC>
    void wide(int) const {
        run<VEC, 64, 1>();  // rows beyond 64 lanes: tiles of one wavefront, the row walked once per tile
    }
};

// the narrowest of 1 / 2 / 4 / 8 / 16 blocks per pass that holds min(B, 16)
template <bool EXPAND, bool ONEHOT>
static void rel_dispatch(const RelArgs& a, int vec, hipStream_t st) {
    const int nb = a.B < kRelBlocks ? a.B : kRelBlocks;
    if (nb <= 1) dispatch_sweep(RelLaunch<EXPAND, ONEHOT, 1>{a, st}, a.F, vec);
    else if (nb <= 2) dispatch_sweep(RelLaunch<EXPAND, ONEHOT, 2>{a, st}, a.F, vec);
    else if (nb <= 4) dispatch_sweep(RelLaunch<EXPAND, ONEHOT, 4>{a, st}, a.F, vec);
    else if (nb <= 8) dispatch_sweep(RelLaunch<EXPAND, ONEHOT, 8>{a, st}, a.F, vec);
    else dispatch_sweep(RelLaunch<EXPAND, ONEHOT, 16>{a, st}, a.F, vec);
}

// The checks the two entry points share; wx / wo: the floats of an input / output row
static int rel_check(const char* who, int64_t nnz, int64_t n_long, int64_t n_slots, const void* items, const void* indices, const void* etype,
                     const void* long_rows, const void* long_ptr, const void* x, const void* out, const void* ws, const void* norm,
                     const void* coef, int64_t ldx, int64_t wx, int64_t ldo, int64_t wo) {
    if (int rc = check_plan(who, items, "items/out", out != nullptr, nnz, "indices/etype/x", indices && etype && x, n_long,
                            "long_rows/long_ptr/workspace", long_rows && long_ptr && ws))
        return rc;
    BOT_REQUIRE(n_long == 0 || n_slots > 0, BOT_E_RANGE, "%s: long rows without slots", who);
    BOT_REQUIRE(out != x, BOT_E_RANGE, "%s: out aliases the input", who);
    BOT_REQUIRE(ldo >= wo && (nnz == 0 || ldx >= wx), BOT_E_RANGE, "%s: row strides smaller than the rows (ldx=%lld < %lld or ldo=%lld < %lld)", who,
                (long long)ldx, (long long)wx, (long long)ldo, (long long)wo);
    BOT_REQUIRE(wo < INT32_MAX && wx < INT32_MAX, BOT_E_RANGE, "%s: B * F exceeds the int32 range", who);
    BOT_REQUIRE(aligned(x, 4) && aligned(out, 4) && aligned(norm, 4) && aligned(coef, 4) && aligned(etype, 4) && aligned(indices, 4) &&
                    aligned(items, 16) && aligned(ws, 16),
                BOT_E_ALIGN, "%s: misaligned pointer", who);
    return 0;
}

}  // namespace bot

extern "C" {

#define REL_COMMON(name)                                                                                                   \
    if (int rc = check_plan_sizes(name, n_rows, nnz, n_items, n_long, n_slots)) return rc;                                 \
    BOT_REQUIRE(F >= 1, BOT_E_RANGE, name ": F=%d (>= 1)", F);                                                             \
    BOT_REQUIRE(R >= 1, BOT_E_RANGE, name ": R=%d relations (>= 1)", R);                                                   \
    BOT_REQUIRE(coef ? B >= 1 : (B == R || B == 0), BOT_E_RANGE, name ": B=%d (>= 1 with coef; R or 0 without: one-hot)", B); \
    const int32_t Bc = coef ? B : R; /* coefficient columns */                                                            \
    if (n_rows == 0) return 0;

int bot_spmm_rel_expand_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                            const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots, const int32_t* etype,
                            const float* norm, const float* coef, int32_t R, int32_t B, const float* x, int64_t ldx, int32_t F, float* out,
                            int64_t ldo, void* workspace, bot_stream_t stream) {
    using namespace bot;
    (void)indptr;
    REL_COMMON("spmm_rel_expand")
    const int64_t wo = (int64_t)Bc * F;
    if (int rc = rel_check("spmm_rel_expand", nnz, n_long, n_slots, items, indices, etype, long_rows, long_ptr, x, out, workspace, norm, coef,
                           ldx, F, ldo, wo))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    const RelArgs a{indices, etype, norm, coef, reinterpret_cast<const int4*>(items), n_items, x, ldx, out, ldo, static_cast<float*>(workspace), F, Bc};
    // (F % vec == 0 keeps every block of a row and every row of the workspace aligned)
    const int vec = pick_vec(F, {ldx, ldo}, {x, out});
    if (coef) rel_dispatch<true, false>(a, vec, st);
    else rel_dispatch<true, true>(a, vec, st);
    if (int rc = hip_status("spmm_rel_expand launch")) return rc;
    if (n_long > 0) {
        launch_sum_combine(a.ws, (int32_t)wo, out, ldo, long_rows, long_ptr, n_long, st);
        if (int rc = hip_status("spmm_rel_expand combine launch")) return rc;
    }
    return 0;
}

int bot_spmm_rel_contract_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                              const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots, const int32_t* etype,
                              const float* norm, const float* coef, int32_t R, int32_t B, const float* y, int64_t ldy, int32_t F, float* out,
                              int64_t ldo, void* workspace, bot_stream_t stream) {
    using namespace bot;
    (void)indptr;
    REL_COMMON("spmm_rel_contract")
    const int64_t wy = (int64_t)Bc * F;
    if (int rc = rel_check("spmm_rel_contract", nnz, n_long, n_slots, items, indices, etype, long_rows, long_ptr, y, out, workspace, norm, coef,
                           ldy, wy, ldo, F))
        return rc;
    hipStream_t st = (hipStream_t)stream;
    const RelArgs a{indices, etype, norm, coef, reinterpret_cast<const int4*>(items), n_items, y, ldy, out, ldo, static_cast<float*>(workspace), F, Bc};
    const int vec = pick_vec(F, {ldy, ldo}, {y, out});
    if (coef) rel_dispatch<false, false>(a, vec, st);
    else {
        const RelArgs one{indices, etype, norm, nullptr, a.items, n_items, y, ldy, out, ldo, a.ws, F, 1};  // one staged block whatever R is
        dispatch_sweep(RelLaunch<false, true, 1>{one, st}, F, vec);
    }
    if (int rc = hip_status("spmm_rel_contract launch")) return rc;
    if (n_long > 0) {
        launch_sum_combine(a.ws, F, out, ldo, long_rows, long_ptr, n_long, st);
        if (int rc = hip_status("spmm_rel_contract combine launch")) return rc;
    }
    return 0;
}

}  // extern "C"
