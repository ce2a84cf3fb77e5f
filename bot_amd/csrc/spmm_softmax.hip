// Softmax-aggregation sweep pair (include/bot_gnn.h "Softmax aggregation") for gfx950: the per-channel softmax aggregator of DeeperGCN
// (Li, Xiong, Thabet, Ghanem, arXiv:2006.07739; bot_amd.nn.GENConv, `ops.copy_u_softmax`).  With m = relu ? max(x, 0) + eps : x,
//   forward   out[v,f] = sum_k a_k m_k,  a_k = exp(beta m_k - lse[v,f]),  lse[v,f] = log sum_k exp(beta m_k),  q[v,f] = sum_k a_k m_k^2
//             over the in-edges k of v (rows = destinations: the CSC); an empty row gives out = lse = q = 0
//   backward  dx[u,f]  = gate_u sum_j dout[v_j,f] exp(beta m_u - lse[v_j,f]) (1 + beta (m_u - out[v_j,f]))       (rows = sources: the CSR)
// beta is ONE float32 read from device memory by every group, so a learnable beta costs no host read.
//
// The gather is the lane-group row sweep that sweep.h describes (walk_row).  A row wider than the group's tile walks feature tiles;
// the ids are read again per tile (sequential, 4 bytes against a 4 F-byte row).
//
// Forward: an online softmax per lane and column, no cross-lane step at all.  Every lane keeps (M, Z, S[, Q]) of its columns in
// registers - M the running maximum of beta m, Z, S, Q the sums of exp(beta m - M) times 1, m, m^2 - and visits the neighbours in
// position order.  ONE exponential per gathered entry: with d = beta m - M, e = exp(-|d|) is the rescale factor of the old sums when
// d > 0 (the entry becomes the maximum, its own weight is 1) and the entry's weight otherwise.  The first neighbour initialises the
// state, so nothing is ever rescaled from -inf.  Epilogue: out = S / Z by a true division (beta = 0: every weight is exactly 1 and
// out is float32(sum) / float32(deg) bit for bit), lse = M + log Z, q = Q / Z.  The chunks of a long row leave their raw state in
// the workspace; spmm_softmax_combine_kernel (one thread per long row and column) folds them in slot order with the same merge and
// applies the same epilogue.  Q exists only in the instances that were asked for q (a beta that requires a gradient: d out / d beta
// = q - out^2, a dense reduction in the caller).
//
// The exponential (smx_exp): v_exp_f32 of t log2(e), corrected to first order by the remainder t - (t log2 e) ln 2 kept with two
// fused multiply-adds, so the rounding of the product - a relative error of 2^-24 |t| in the result, 6e-6 at t = -100 - is gone; a
// result below 2^-126 is flushed to 0 by the instruction (its weight is below 1e-38 of the row's largest, which is 1).
//
// Backward: the row owner holds m_u, beta m_u and the gate x[u,f] > 0 (torch's ReLU convention: 0 at x == 0); per out-edge three row
// gathers of the destination (dout, out, lse) and one exponential per entry; nothing is stored per edge, so no csr2csc.  The sum runs in
// position order in registers, long rows chunk by chunk into `partial` and through the slot-order combine.
// No atomics in either direction: the bytes repeat from call to call.
//
// HBM model: forward 4 * [E * (1 + F) + n_dst * F * (2 or 3)] bytes (ids and source rows per edge; out, lse and - when asked for - q
// per row): the sum sweep's plus the statistics' stores.  Backward 4 * [E * (1 + 3 F) + 2 * n_src * F] (ids and three destination rows
// per edge; x and dx per row): three times the transposed sum sweep's gather.
#include "sweep.h"

#include <cmath>
#include <initializer_list>

// Every product below is rounded on its own and every fused multiply-add is written out (smx.h switches contraction off): the instances
// with and without q, the chunks and the combine then run the same arithmetic, so they give the same bytes, and beta * m is the same
// float32 wherever it is formed.
#include "smx.h"

namespace bot {

// (the message's select smx_message, SmxArgs and the state's way out, BOT_SMX_FINISH_TILE: smx.h, shared with spmm_softmax_edge.hip)
template <bool WQ, int VEC, int LANES, int NCHUNK>
__global__ __launch_bounds__(kBlock) void spmm_softmax_kernel(SmxArgs a) {
    constexpr int TILE = LANES * VEC * NCHUNK;
    const int lane = threadIdx.x % LANES;
    const int64_t item = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / LANES;
    if (item >= a.n_items) return;  // whole groups leave together
    const RowItem it = load_item<LANES>(a.items, item);
    const float beta = *a.beta;
    const bool relu = a.relu != 0;
    const float eps = a.eps;
    for (int col0 = 0; col0 < a.F; col0 += TILE) {  // groups narrower than a wavefront have one tile (SmxLaunch)
        const ColTile<VEC, LANES, NCHUNK> tile(col0, lane, a.F);
        float M[NCHUNK][VEC] = {}, Z[NCHUNK][VEC] = {}, S[NCHUNK][VEC] = {}, Q[NCHUNK][VEC] = {};
        walk_row<LANES, float[NCHUNK][VEC]>(
            it.beg, it.end, lane, [&](int k, bool in) { return Edge{in ? a.indices[k] : 0, 0}; },
            [&](int s, int, float (&v)[NCHUNK][VEC], int) {
                const float* p = a.x + (int64_t)s * a.ldx;
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c) vload<VEC>(v[c], p + tile.off[c]);
            },
            [&](int, int, const float (&v)[NCHUNK][VEC], int k) {
                if (k == it.beg) {  // the first neighbour is the state
#pragma unroll
                    for (int c = 0; c < NCHUNK; ++c)
#pragma unroll
                        for (int t = 0; t < VEC; ++t) {
                            const float m = smx_message(v[c][t], relu, eps);
                            M[c][t] = beta * m;
                            Z[c][t] = 1.f;
                            S[c][t] = m;
                            Q[c][t] = m * m;
                        }
                    return;
                }
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c)
#pragma unroll
                    for (int t = 0; t < VEC; ++t) {
                        const float m = smx_message(v[c][t], relu, eps);
                        smx_merge<WQ>(M[c][t], Z[c][t], S[c][t], Q[c][t], beta * m, 1.f, m, m * m);
                    }
            });
        BOT_SMX_FINISH_TILE();  // a chunk of a long row: the raw state into the workspace; else the row's epilogue
    }
}

// One thread per (long row, column): the chunks' states are folded in slot order (= position order) with the sweep's merge, then the
// row's epilogue.  (A long row has at least two chunks and no chunk is empty.)
template <bool WQ>
__global__ __launch_bounds__(kBlock) void spmm_softmax_combine_kernel(SmxArgs a, const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long) {
    const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gid >= n_long * a.F) return;
    const int64_t i = gid / a.F;
    const int c = (int)(gid - i * a.F);
    const int row = long_rows[i], p1 = long_ptr[i + 1];
    int s = long_ptr[i];
    float M = 0.f, Z = 0.f, S = 0.f, Q = 0.f;
    const bool some = s < p1;
    if (some) {
        const float* w = a.ws + (int64_t)s * a.F + c;
        M = w[0], Z = w[a.plane], S = w[2 * a.plane];
        if constexpr (WQ) Q = w[3 * a.plane];
        ++s;
    }
    for (; s < p1; ++s) {
        const float* w = a.ws + (int64_t)s * a.F + c;
        float Q2 = 0.f;
        if constexpr (WQ) Q2 = w[3 * a.plane];
        smx_merge<WQ>(M, Z, S, Q, w[0], w[a.plane], w[2 * a.plane], Q2);
    }
    a.out[(int64_t)row * a.ldo + c] = some ? S / Z : 0.f;
    a.lse[(int64_t)row * a.ldl + c] = some ? M + logf(Z) : 0.f;
    if constexpr (WQ) a.q[(int64_t)row * a.ldq + c] = some ? Q / Z : 0.f;
}

struct SmxBwdArgs {
    const int32_t* indices;
    const int4* items;
    int64_t n_items;
    const float* x;
    int64_t ldx;
    const float* beta;
    int32_t relu;
    float eps;
    const float* dout;
    int64_t ldd;
    const float* out;
    int64_t ldo;
    const float* lse;
    int64_t ldl;
    int32_t F;
    float* dx;
    int64_t lddx;
    float* partial;  // [n_slots, F] chunk sums
};

template <int VEC, int NCHUNK>
struct SmxBwdStage {
    float d[NCHUNK][VEC], o[NCHUNK][VEC], l[NCHUNK][VEC];
};

template <int VEC, int LANES, int NCHUNK>
__global__ __launch_bounds__(kBlock) void spmm_softmax_bwd_kernel(SmxBwdArgs a) {
    constexpr int TILE = LANES * VEC * NCHUNK;
    const int lane = threadIdx.x % LANES;
    const int64_t item = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / LANES;
    if (item >= a.n_items) return;  // whole groups leave together
    const RowItem it = load_item<LANES>(a.items, item);
    const float beta = *a.beta;
    const bool relu = a.relu != 0;
    for (int col0 = 0; col0 < a.F; col0 += TILE) {
        const ColTile<VEC, LANES, NCHUNK> tile(col0, lane, a.F);
        float m[NCHUNK][VEC], bm[NCHUNK][VEC], acc[NCHUNK][VEC] = {};
        bool gate[NCHUNK][VEC];
#pragma unroll
        for (int c = 0; c < NCHUNK; ++c) {
            float xv[VEC];
            vload<VEC>(xv, a.x + (int64_t)it.row * a.ldx + tile.off[c]);
#pragma unroll
            for (int t = 0; t < VEC; ++t) {
                m[c][t] = smx_message(xv[t], relu, a.eps);
                bm[c][t] = beta * m[c][t];
                gate[c][t] = !relu || xv[t] > 0.f;
            }
        }
        walk_row<LANES, SmxBwdStage<VEC, NCHUNK>>(
            it.beg, it.end, lane, [&](int k, bool in) { return Edge{in ? a.indices[k] : 0, 0}; },
            [&](int s, int, SmxBwdStage<VEC, NCHUNK>& g, int) {
                const float* pd = a.dout + (int64_t)s * a.ldd;
                const float* po = a.out + (int64_t)s * a.ldo;
                const float* pl = a.lse + (int64_t)s * a.ldl;
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c) {
                    vload<VEC>(g.d[c], pd + tile.off[c]);
                    vload<VEC>(g.o[c], po + tile.off[c]);
                    vload<VEC>(g.l[c], pl + tile.off[c]);
                }
            },
            [&](int, int, const SmxBwdStage<VEC, NCHUNK>& g, int) {
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c)
#pragma unroll
                    for (int t = 0; t < VEC; ++t) {
                        const float w = smx_exp(bm[c][t] - g.l[c][t]);
                        acc[c][t] = fmaf(g.d[c][t] * w, fmaf(beta, m[c][t] - g.o[c][t], 1.f), acc[c][t]);
                    }
            });
#pragma unroll
        for (int c = 0; c < NCHUNK; ++c)
#pragma unroll
            for (int t = 0; t < VEC; ++t) acc[c][t] = gate[c][t] ? acc[c][t] : 0.f;  // a select: a gated entry is 0 whatever the sum holds
        tile.store(sum_row(it, a.dx, a.lddx, a.partial, a.F), acc);
    }
}

template <bool WQ>
struct SmxLaunch {
    const SmxArgs& a;
    hipStream_t st;
    template <int VEC, int LANES, int NCHUNK>
    void run() const {
        const int64_t blocks = (a.n_items * LANES + kBlock - 1) / kBlock;
        if (blocks == 0) return;
        set_kernel(WQ ? "bot::spmm_softmax_kernel<q,%d,%d,%d>" : "bot::spmm_softmax_kernel<%d,%d,%d>", VEC, LANES, NCHUNK);
        hipLaunchKernelGGL((spmm_softmax_kernel<WQ, VEC, LANES, NCHUNK>), dim3((unsigned)blocks), dim3(kBlock), 0, st, a);
    }
    template <int VEC>
    void wide(int) const {
        run<VEC, 64, 2>();  // wider rows walk tiles of 128 lanes
    }
};

struct SmxBwdLaunch {
    const SmxBwdArgs& a;
    hipStream_t st;
    template <int VEC, int LANES, int NCHUNK>
    void run() const {
        const int64_t blocks = (a.n_items * LANES + kBlock - 1) / kBlock;
        if (blocks == 0) return;
        set_kernel("bot::spmm_softmax_bwd_kernel<%d,%d,%d>", VEC, LANES, NCHUNK);
        hipLaunchKernelGGL((spmm_softmax_bwd_kernel<VEC, LANES, NCHUNK>), dim3((unsigned)blocks), dim3(kBlock), 0, st, a);
    }
    template <int VEC>
    void wide(int) const {
        run<VEC, 64, 1>();  // three staged rows per neighbour in flight: tiles of 64 lanes keep the registers of four of them
    }
};

void launch_smx_combine(const SmxArgs& a, const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, hipStream_t st) {
    const dim3 grid((unsigned)((n_long * a.F + kBlock - 1) / kBlock));
    if (a.q) hipLaunchKernelGGL(spmm_softmax_combine_kernel<true>, grid, dim3(kBlock), 0, st, a, long_rows, long_ptr, n_long);
    else hipLaunchKernelGGL(spmm_softmax_combine_kernel<false>, grid, dim3(kBlock), 0, st, a, long_rows, long_ptr, n_long);
}

}  // namespace bot

extern "C" {

int bot_spmm_softmax_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                         const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots, const float* x, int64_t ldx, int32_t F,
                         const float* beta, int32_t relu, float eps, float* out, int64_t ldo, float* lse, int64_t ldl, float* q, int64_t ldq,
                         void* workspace, bot_stream_t stream) {
    using namespace bot;
    (void)indptr;
    if (int rc = check_plan_sizes("spmm_softmax", n_rows, nnz, n_items, n_long, n_slots)) return rc;
    BOT_REQUIRE(F >= 1, BOT_E_RANGE, "spmm_softmax: F=%d (>= 1)", F);
    BOT_REQUIRE(std::isfinite(eps), BOT_E_RANGE, "spmm_softmax: eps is not finite");
    if (n_rows == 0) return 0;
    if (int rc = check_plan("spmm_softmax", items, "items/x/beta/out/lse", x && beta && out && lse, nnz, "indices", indices, n_long,
                            "long_rows/long_ptr/workspace", long_rows && long_ptr && workspace))
        return rc;
    BOT_REQUIRE(n_long == 0 || n_slots > 0, BOT_E_RANGE, "spmm_softmax: long rows without slots");
    BOT_REQUIRE(out != x && lse != x && q != x && out != lse && out != q && lse != q, BOT_E_RANGE,
                "spmm_softmax: out, lse and q alias x or each other");
    BOT_REQUIRE(ldx >= F && ldo >= F && ldl >= F && (!q || ldq >= F), BOT_E_RANGE,
                "spmm_softmax: row strides smaller than F=%d (ldx=%lld ldo=%lld ldl=%lld ldq=%lld)", F, (long long)ldx, (long long)ldo,
                (long long)ldl, (long long)ldq);
    BOT_REQUIRE(aligned(x, 4) && aligned(beta, 4) && aligned(out, 4) && aligned(lse, 4) && aligned(q, 4) && aligned(items, 16) &&
                    aligned(workspace, 16),
                BOT_E_ALIGN, "spmm_softmax: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    const SmxArgs a{indices, reinterpret_cast<const int4*>(items), n_items, x, ldx, beta, F, relu, eps, out, ldo, lse, ldl, q, q ? ldq : F,
                    static_cast<float*>(workspace), n_slots * F};
    // (the workspace: 16-byte base, planes of n_slots * F floats, slot rows of F floats - F % vec == 0 keeps every row aligned)
    const int vec = pick_vec(F, {ldx, ldo, ldl, a.ldq}, {x, out, lse, q});
    if (q) dispatch_sweep(SmxLaunch<true>{a, st}, F, vec);
    else dispatch_sweep(SmxLaunch<false>{a, st}, F, vec);
    if (int rc = hip_status("spmm_softmax launch")) return rc;
    if (n_long > 0) {
        launch_smx_combine(a, long_rows, long_ptr, n_long, st);
        if (int rc = hip_status("spmm_softmax combine launch")) return rc;
    }
    return 0;
}

int bot_spmm_softmax_bwd_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                             const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, const float* x, int64_t ldx, const float* beta,
                             int32_t relu, float eps, const float* dout, int64_t ldd, const float* out, int64_t ldo, const float* lse, int64_t ldl,
                             int32_t F, float* dx, int64_t lddx, float* partial, bot_stream_t stream) {
    using namespace bot;
    (void)indptr;
    if (int rc = check_plan_sizes("spmm_softmax_bwd", n_rows, nnz, n_items, n_long)) return rc;
    BOT_REQUIRE(F >= 1, BOT_E_RANGE, "spmm_softmax_bwd: F=%d (>= 1)", F);
    BOT_REQUIRE(std::isfinite(eps), BOT_E_RANGE, "spmm_softmax_bwd: eps is not finite");
    if (n_rows == 0) return 0;
    if (int rc = check_plan("spmm_softmax_bwd", items, "items/x/beta/dx", x && beta && dx, nnz, "indices/dout/out/lse",
                            indices && dout && out && lse, n_long, "long_rows/long_ptr/partial", long_rows && long_ptr && partial))
        return rc;
    BOT_REQUIRE(dx != x && dx != dout && dx != out && dx != lse, BOT_E_RANGE, "spmm_softmax_bwd: dx aliases an input");
    BOT_REQUIRE(ldx >= F && ldd >= F && ldo >= F && ldl >= F && lddx >= F, BOT_E_RANGE,
                "spmm_softmax_bwd: row strides smaller than F=%d (ldx=%lld ldd=%lld ldo=%lld ldl=%lld lddx=%lld)", F, (long long)ldx,
                (long long)ldd, (long long)ldo, (long long)ldl, (long long)lddx);
    BOT_REQUIRE(aligned(x, 4) && aligned(beta, 4) && aligned(dout, 4) && aligned(out, 4) && aligned(lse, 4) && aligned(dx, 4) &&
                    aligned(items, 16) && aligned(partial, 16),
                BOT_E_ALIGN, "spmm_softmax_bwd: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    const SmxBwdArgs a{indices, reinterpret_cast<const int4*>(items), n_items, x, ldx, beta, relu, eps, dout, ldd, out, ldo, lse, ldl, F, dx,
                       lddx, partial};
    const int vec = pick_vec(F, {ldx, ldd, ldo, ldl, lddx}, {x, dout, out, lse, dx});
    dispatch_sweep(SmxBwdLaunch{a, st}, F, vec);
    if (int rc = hip_status("spmm_softmax_bwd launch")) return rc;
    if (n_long > 0) {
        launch_sum_combine(partial, F, dx, lddx, long_rows, long_ptr, n_long, st);
        if (int rc = hip_status("spmm_softmax_bwd combine launch")) return rc;
    }
    return 0;
}

}  // extern "C"
