// Softmax aggregation with raw edge features (include/bot_gnn.h "Softmax aggregation with edge features") for gfx950: DeeperGCN's message
// with the edge encoder folded into the sweep (bot_amd.nn.GENConv(edge_dim=K), `ops.u_add_e_softmax`).  For an edge e = (u -> v):
//   z_e = x[u,f] + ((ef[e,0] wt[0,f] + ... + ef[e,K-1] wt[K-1,f]) + bias[f])      the sum in index order as a chain of fused multiply-adds
//         (its first term a rounded product), then the bias, then x: K + 2 roundings.  edge_z below is the ONE place that forms it.
//   m_e = relu ? (z_e < 0 ? 0 : z_e) + eps : z_e                                   (smx_message)
//   forward   out, lse, q of spmm_softmax.hip over the m_e of a destination's in-edges (rows = destinations: the CSC)
//   backward  dz_e = gate_e dout[v,f] a c,  a = exp(beta m_e - lse[v,f]),  c = 1 + beta (m_e - out[v,f]),  gate_e = !relu || z_e > 0
//             dx[u,f] = sum over the out-edges of u of dz_e;   dweight[f,j] = sum over all edges of ef[e,j] dz_e       (rows = sources: the CSR)
// ef is [E, K] raw floats, K <= 16, read at row eperm[k] of position k (NULL: k itself), so the encoded [E, F] operand never exists:
// an edge streams 4 K bytes beside its 4 F-byte source row.  wt is the encoder's weight transposed to [K, F], so that a lane's columns
// are contiguous; the lane keeps its K x VEC slice of it (KP x VEC registers, KP = 4 / 8 / 16 the instance's padded K: the padding
// holds zeros, which add +0 to the chain) and its VEC biases for the whole sweep.
//
// Forward: spmm_softmax_kernel's walk and online softmax.  `read` hands the ef row of a position as the Edge word, `fetch` loads the K
// floats of that row (a group-uniform address; 16-byte loads where K % 4 == 0 and ef is 16-byte aligned) beside the source row, `use`
// forms z.  Everything behind m is smx.h's: the merge, the state's way out (BOT_SMX_FINISH_TILE), the long rows' workspace and combine
// (launch_smx_combine).  Rows wider than 64 lanes walk tiles of 64 lanes, so that one tile's slice of wt is live.
//
// Backward: one persistent sweep.  Feature tiles of LANES * VEC columns lie on grid.y, so a lane owns the same columns for every item it
// sees; the groups of a workgroup stride over the plan's items (item = blockIdx.x * G + group, + gridDim.x * G, ...).  The row owner holds
// x[u]; per out-edge the three destination gathers of spmm_softmax_bwd_kernel plus the ef row; z, m and the gate are formed again per
// edge with edge_z.  dx goes through sum_row / launch_sum_combine as there.  dweight: every lane keeps KP x VEC partial sums over all
// the edges its group visits (position order within an item, items in stride order); at the end the workgroup's groups are added in
// group order through LDS, one j at a time, and the workgroup writes its [K, tile] partial to dw_ws [grid.x, K, F]; a second kernel adds
// the workgroups in index order into dweight [F, K].  grid.x is a pure function of (n_items, F, vec) with a fixed cap (edge_bwd_blocks),
// never of the device: no float atomics, and two calls give the same bytes.  The instances without dweight carry no partials.
//
// HBM model: forward 4 * [E * (1 + K + F) + n_dst * F * (2 or 3)] bytes (+ 4 E with an eperm); backward 4 * [E * (2 + K + 3 F) + 2 *
// n_src * F] bytes plus the partials, 4 * grid.x * K * F written and read once.
#include "sweep.h"

#include <cmath>
#include <initializer_list>

// As in spmm_softmax.hip: every product is rounded on its own and every fused multiply-add is written out (smx.h switches contraction off
// for the rest of this file), so the forward and the backward form the same z and the same beta * m.
#include "smx.h"
#include "edge_term.h"

namespace bot {

// z of the contract: the chain over j in index order, then the bias, then x
template <int KP, int VEC>
__device__ __forceinline__ float edge_z(float x, const float (&e)[KP], const float (&w)[KP][VEC], float b, int t) {
    return x + (edge_chain<KP, VEC>(e, w, t) + b);
}

struct SmxEdgeOperands {
    const float* ef;       // [E, K]
    const int32_t* eperm;  // [nnz] the row of ef of a position, or NULL: the position
    const float* wt;       // [K, F]
    const float* bias;     // [F] or NULL
    int32_t K;
    int32_t k4;            // ef rows are read with 16-byte loads
};

template <int KP, int VEC>
struct SmxEdgeStage {
    float v[1][VEC];
    float e[KP];
};

template <bool WQ, int KP, int VEC, int LANES>
__global__ __launch_bounds__(kBlock) void spmm_softmax_edge_kernel(SmxArgs a, SmxEdgeOperands o) {
    constexpr int NCHUNK = 1, TILE = LANES * VEC;
    constexpr int U = KP > 8 ? 2 : 4;  // the staged ef rows of four neighbours would not fit beside the slice of wt at KP = 16
    const int lane = threadIdx.x % LANES;
    const int64_t item = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / LANES;
    if (item >= a.n_items) return;  // whole groups leave together
    const RowItem it = load_item<LANES>(a.items, item);
    const float beta = *a.beta;
    const bool relu = a.relu != 0;
    const float eps = a.eps;
    const int K = o.K;
    const bool k4 = o.k4 != 0;
    for (int col0 = 0; col0 < a.F; col0 += TILE) {  // groups narrower than a wavefront have one tile
        const ColTile<VEC, LANES, 1> tile(col0, lane, a.F);
        float w[KP][VEC], b[VEC];
        load_slice<KP, VEC>(w, b, o.wt, o.bias, K, a.F, tile.off[0]);
        float M[1][VEC] = {}, Z[1][VEC] = {}, S[1][VEC] = {}, Q[1][VEC] = {};
        walk_row<LANES, SmxEdgeStage<KP, VEC>, U>(
            it.beg, it.end, lane, [&](int k, bool in) { return Edge{in ? a.indices[k] : 0, in ? (o.eperm ? o.eperm[k] : k) : 0}; },
            [&](int s, int r, SmxEdgeStage<KP, VEC>& g, int) {
                vload<VEC>(g.v[0], a.x + (int64_t)s * a.ldx + tile.off[0]);
                load_ef<KP>(g.e, o.ef + (int64_t)r * K, K, k4);
            },
            [&](int, int, const SmxEdgeStage<KP, VEC>& g, int k) {
                if (k == it.beg) {  // the first neighbour is the state
#pragma unroll
                    for (int t = 0; t < VEC; ++t) {
                        const float m = smx_message(edge_z<KP, VEC>(g.v[0][t], g.e, w, b[t], t), relu, eps);
                        M[0][t] = beta * m;
                        Z[0][t] = 1.f;
                        S[0][t] = m;
                        Q[0][t] = m * m;
                    }
                    return;
                }
#pragma unroll
                for (int t = 0; t < VEC; ++t) {
                    const float m = smx_message(edge_z<KP, VEC>(g.v[0][t], g.e, w, b[t], t), relu, eps);
                    smx_merge<WQ>(M[0][t], Z[0][t], S[0][t], Q[0][t], beta * m, 1.f, m, m * m);
                }
            });
        BOT_SMX_FINISH_TILE();  // a chunk of a long row: the raw state into the workspace; else the row's epilogue
    }
}

struct SmxEdgeBwdArgs {
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
    float* dx;       // NULL: not computed
    int64_t lddx;
    float* partial;  // [n_slots, F] chunk sums of dx
    float* dw_ws;    // [gridDim.x, K, F] the workgroups' partials of dweight (the instances with WD)
};

template <int KP, int VEC>
struct SmxEdgeBwdStage {
    float d[VEC], o[VEC], l[VEC];
    float e[KP];
};

template <bool WD, int KP, int VEC, int LANES>
__global__ __launch_bounds__(kBlock) void spmm_softmax_edge_bwd_kernel(SmxEdgeBwdArgs a, SmxEdgeOperands o) {
    constexpr int TILE = LANES * VEC, G = kBlock / LANES;
    constexpr int U = KP > 8 ? 2 : 4;
    __shared__ float red[WD ? kBlock * VEC : 1];
    const int lane = threadIdx.x % LANES, grp = threadIdx.x / LANES;
    const float beta = *a.beta;
    const bool relu = a.relu != 0;
    const int K = o.K;
    const bool k4 = o.k4 != 0;
    const ColTile<VEC, LANES, 1> tile((int)blockIdx.y * TILE, lane, a.F);
    float w[KP][VEC], b[VEC], dw[WD ? KP : 1][VEC] = {};
    load_slice<KP, VEC>(w, b, o.wt, o.bias, K, a.F, tile.off[0]);
    // no thread leaves before the end: the fold below is a workgroup's
    for (int64_t item = (int64_t)blockIdx.x * G + grp; item < a.n_items; item += (int64_t)gridDim.x * G) {
        const RowItem it = load_item<LANES>(a.items, item);
        float xv[VEC], acc[1][VEC] = {};
        vload<VEC>(xv, a.x + (int64_t)it.row * a.ldx + tile.off[0]);
        walk_row<LANES, SmxEdgeBwdStage<KP, VEC>, U>(
            it.beg, it.end, lane, [&](int k, bool in) { return Edge{in ? a.indices[k] : 0, in ? (o.eperm ? o.eperm[k] : k) : 0}; },
            [&](int s, int r, SmxEdgeBwdStage<KP, VEC>& g, int) {
                vload<VEC>(g.d, a.dout + (int64_t)s * a.ldd + tile.off[0]);
                vload<VEC>(g.o, a.out + (int64_t)s * a.ldo + tile.off[0]);
                vload<VEC>(g.l, a.lse + (int64_t)s * a.ldl + tile.off[0]);
                load_ef<KP>(g.e, o.ef + (int64_t)r * K, K, k4);
            },
            [&](int, int, const SmxEdgeBwdStage<KP, VEC>& g, int) {
#pragma unroll
                for (int t = 0; t < VEC; ++t) {
                    const float z = edge_z<KP, VEC>(xv[t], g.e, w, b[t], t);
                    const float m = smx_message(z, relu, a.eps);
                    const bool gate = !relu || z > 0.f;
                    const float da = g.d[t] * smx_exp(beta * m - g.l[t]);
                    const float c = fmaf(beta, m - g.o[t], 1.f);
                    acc[0][t] = gate ? fmaf(da, c, acc[0][t]) : acc[0][t];  // a select: a gated edge adds nothing whatever its term holds
                    if constexpr (WD) {
                        const float dz = gate ? da * c : 0.f;
#pragma unroll
                        for (int j = 0; j < KP; ++j) dw[j][t] = fmaf(g.e[j], dz, dw[j][t]);
                    }
                }
            });
        if (a.dx) tile.store(sum_row(it, a.dx, a.lddx, a.partial, a.F), acc);
    }
    if constexpr (WD) {
#pragma unroll
        for (int j = 0; j < KP; ++j)
            if (j < K) {  // uniform
                vstore<VEC>(red + threadIdx.x * VEC, dw[j]);
                __syncthreads();
                if (grp == 0 && tile.act[0]) {
                    float s[VEC];
#pragma unroll
                    for (int t = 0; t < VEC; ++t) s[t] = red[lane * VEC + t];
                    for (int g2 = 1; g2 < G; ++g2)  // group order
#pragma unroll
                        for (int t = 0; t < VEC; ++t) s[t] += red[(g2 * LANES + lane) * VEC + t];
                    vstore<VEC>(a.dw_ws + ((int64_t)blockIdx.x * K + j) * a.F + tile.off[0], s);
                }
                __syncthreads();
            }
    }
}

// dweight[f, j] = dw_ws[0, j, f] + dw_ws[1, j, f] + ... in workgroup order; one thread per (j, f)
__global__ __launch_bounds__(kBlock) void spmm_softmax_edge_dw_kernel(const float* ws, int64_t n_blocks, int32_t K, int32_t F, float* dweight) {
    const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gid >= (int64_t)K * F) return;
    const int j = (int)(gid / F), f = (int)(gid - (int64_t)j * F);
    float s = 0.f;
    for (int64_t i = 0; i < n_blocks; ++i) s += ws[(i * K + j) * F + f];
    dweight[(int64_t)f * K + j] = s;
}

template <bool WQ>
struct SmxEdgeLaunch {
    const SmxArgs& a;
    const SmxEdgeOperands& o;
    hipStream_t st;
    template <int KP>
    struct At {
        const SmxEdgeLaunch& l;
        template <int VEC, int LANES, int NCHUNK>
        void run() const {
            const int64_t blocks = (l.a.n_items * LANES + kBlock - 1) / kBlock;
            if (blocks == 0) return;
            set_kernel(WQ ? "bot::spmm_softmax_edge_kernel<q,%d,%d,%d>" : "bot::spmm_softmax_edge_kernel<%d,%d,%d>", KP, VEC, LANES);
            hipLaunchKernelGGL((spmm_softmax_edge_kernel<WQ, KP, VEC, LANES>), dim3((unsigned)blocks), dim3(kBlock), 0, l.st, l.a, l.o);
        }
        template <int VEC>
        void wide(int) const {
            run<VEC, 64, 1>();  // wider rows walk tiles of 64 lanes: one tile's slice of wt is live
        }
    };
};

template <bool WD>
struct SmxEdgeBwdLaunch {
    const SmxEdgeBwdArgs& a;
    const SmxEdgeOperands& o;
    int64_t dw_rows;   // the workgroup partials dw_ws holds
    int64_t* used;     // grid.x of the launch, 0 when the workspace is too small
    hipStream_t st;
    template <int KP>
    struct At {
        const SmxEdgeBwdLaunch& l;
        template <int VEC, int LANES, int NCHUNK>
        void run() const {
            const int64_t n_tiles = (l.a.F + LANES * VEC - 1) / (LANES * VEC);
            const int64_t bx = edge_bwd_blocks(l.a.n_items, LANES, n_tiles);
            if (WD && bx > l.dw_rows) {
                *l.used = -bx;
                return;
            }
            *l.used = bx;
            set_kernel(WD ? "bot::spmm_softmax_edge_bwd_kernel<dw,%d,%d,%d>" : "bot::spmm_softmax_edge_bwd_kernel<%d,%d,%d>", KP, VEC, LANES);
            hipLaunchKernelGGL((spmm_softmax_edge_bwd_kernel<WD, KP, VEC, LANES>), dim3((unsigned)bx, (unsigned)n_tiles), dim3(kBlock), 0, l.st,
                               l.a, l.o);
        }
        template <int VEC>
        void wide(int) const {
            run<VEC, 64, 1>();
        }
    };
};

static int check_edge_operands(const char* who, int64_t nnz, const float* ef, int32_t K, const float* wt, const float* bias) {
    BOT_REQUIRE(K >= 1 && K <= kEdgeMaxK, BOT_E_RANGE, "%s: K=%d (1 .. %d)", who, K, kEdgeMaxK);
    BOT_REQUIRE(wt && (nnz == 0 || ef), BOT_E_NULL, "%s: ef/wt is NULL", who);
    BOT_REQUIRE(aligned(ef, 4) && aligned(wt, 4) && aligned(bias, 4), BOT_E_ALIGN, "%s: misaligned pointer", who);
    return 0;
}

}  // namespace bot

extern "C" {

int bot_spmm_softmax_edge_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                              const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots, const float* x, int64_t ldx,
                              int32_t F, const float* ef, int32_t K, const int32_t* eperm, const float* wt, const float* bias, const float* beta,
                              int32_t relu, float eps, float* out, int64_t ldo, float* lse, int64_t ldl, float* q, int64_t ldq, void* workspace,
                              bot_stream_t stream) {
    using namespace bot;
    (void)indptr;
    if (int rc = check_plan_sizes("spmm_softmax_edge", n_rows, nnz, n_items, n_long, n_slots)) return rc;
    BOT_REQUIRE(F >= 1, BOT_E_RANGE, "spmm_softmax_edge: F=%d (>= 1)", F);
    BOT_REQUIRE(std::isfinite(eps), BOT_E_RANGE, "spmm_softmax_edge: eps is not finite");
    if (int rc = check_edge_operands("spmm_softmax_edge", nnz, ef, K, wt, bias)) return rc;
    if (n_rows == 0) return 0;
    if (int rc = check_plan("spmm_softmax_edge", items, "items/x/beta/out/lse", x && beta && out && lse, nnz, "indices", indices, n_long,
                            "long_rows/long_ptr/workspace", long_rows && long_ptr && workspace))
        return rc;
    BOT_REQUIRE(n_long == 0 || n_slots > 0, BOT_E_RANGE, "spmm_softmax_edge: long rows without slots");
    BOT_REQUIRE(out != x && lse != x && q != x && out != lse && out != q && lse != q, BOT_E_RANGE,
                "spmm_softmax_edge: out, lse and q alias x or each other");
    BOT_REQUIRE(ldx >= F && ldo >= F && ldl >= F && (!q || ldq >= F), BOT_E_RANGE,
                "spmm_softmax_edge: row strides smaller than F=%d (ldx=%lld ldo=%lld ldl=%lld ldq=%lld)", F, (long long)ldx, (long long)ldo,
                (long long)ldl, (long long)ldq);
    BOT_REQUIRE(aligned(x, 4) && aligned(beta, 4) && aligned(out, 4) && aligned(lse, 4) && aligned(q, 4) && aligned(eperm, 4) &&
                    aligned(items, 16) && aligned(workspace, 16),
                BOT_E_ALIGN, "spmm_softmax_edge: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    const SmxArgs a{indices, reinterpret_cast<const int4*>(items), n_items, x, ldx, beta, F, relu, eps, out, ldo, lse, ldl, q, q ? ldq : F,
                    static_cast<float*>(workspace), n_slots * F};
    const SmxEdgeOperands o{ef, eperm, wt, bias, K, (K % 4 == 0 && aligned(ef, 16)) ? 1 : 0};
    const int vec = pick_vec(F, {ldx, ldo, ldl, a.ldq}, {x, out, lse, q, wt, bias});
    if (q) dispatch_kp(SmxEdgeLaunch<true>{a, o, st}, K, F, vec);
    else dispatch_kp(SmxEdgeLaunch<false>{a, o, st}, K, F, vec);
    if (int rc = hip_status("spmm_softmax_edge launch")) return rc;
    if (n_long > 0) {
        launch_smx_combine(a, long_rows, long_ptr, n_long, st);
        if (int rc = hip_status("spmm_softmax_edge combine launch")) return rc;
    }
    return 0;
}

int bot_spmm_softmax_edge_bwd_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items,
                                  int64_t n_items, const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, const float* x, int64_t ldx,
                                  const float* ef, int32_t K, const int32_t* eperm, const float* wt, const float* bias, const float* beta,
                                  int32_t relu, float eps, const float* dout, int64_t ldd, const float* out, int64_t ldo, const float* lse,
                                  int64_t ldl, int32_t F, float* dx, int64_t lddx, float* partial, float* dweight, float* dw_workspace,
                                  int64_t dw_rows, bot_stream_t stream) {
    using namespace bot;
    (void)indptr;
    if (int rc = check_plan_sizes("spmm_softmax_edge_bwd", n_rows, nnz, n_items, n_long)) return rc;
    BOT_REQUIRE(F >= 1, BOT_E_RANGE, "spmm_softmax_edge_bwd: F=%d (>= 1)", F);
    BOT_REQUIRE(std::isfinite(eps), BOT_E_RANGE, "spmm_softmax_edge_bwd: eps is not finite");
    BOT_REQUIRE(dw_rows >= 0, BOT_E_RANGE, "spmm_softmax_edge_bwd: negative size");
    if (int rc = check_edge_operands("spmm_softmax_edge_bwd", nnz, ef, K, wt, bias)) return rc;
    if (!dx && !dweight) return 0;
    hipStream_t st = (hipStream_t)stream;
    BOT_REQUIRE(aligned(dweight, 4), BOT_E_ALIGN, "spmm_softmax_edge_bwd: misaligned pointer");
    if (n_rows == 0) {  // no edge: dweight is zero, dx has no rows
        if (dweight) {
            (void)hipMemsetAsync(dweight, 0, sizeof(float) * (size_t)K * (size_t)F, st);
            if (int rc = hip_status("spmm_softmax_edge_bwd memset")) return rc;
        }
        return 0;
    }
    if (int rc = check_plan("spmm_softmax_edge_bwd", items, "items/x/beta", x && beta, nnz, "indices/dout/out/lse", indices && dout && out && lse,
                            dx ? n_long : 0, "long_rows/long_ptr/partial", long_rows && long_ptr && partial))
        return rc;
    BOT_REQUIRE(!dweight || dw_workspace, BOT_E_NULL, "spmm_softmax_edge_bwd: dweight needs dw_workspace");
    BOT_REQUIRE(!dx || (dx != x && dx != dout && dx != out && dx != lse), BOT_E_RANGE, "spmm_softmax_edge_bwd: dx aliases an input");
    BOT_REQUIRE(ldx >= F && ldd >= F && ldo >= F && ldl >= F && (!dx || lddx >= F), BOT_E_RANGE,
                "spmm_softmax_edge_bwd: row strides smaller than F=%d (ldx=%lld ldd=%lld ldo=%lld ldl=%lld lddx=%lld)", F, (long long)ldx,
                (long long)ldd, (long long)ldo, (long long)ldl, (long long)lddx);
    BOT_REQUIRE(aligned(x, 4) && aligned(beta, 4) && aligned(dout, 4) && aligned(out, 4) && aligned(lse, 4) && aligned(dx, 4) &&
                    aligned(eperm, 4) && aligned(items, 16) && aligned(partial, 16) && aligned(dw_workspace, 16),
                BOT_E_ALIGN, "spmm_softmax_edge_bwd: misaligned pointer");
    const SmxEdgeBwdArgs a{indices, reinterpret_cast<const int4*>(items), n_items, x, ldx, beta, relu, eps, dout, ldd, out, ldo, lse, ldl, F, dx,
                           dx ? lddx : F, partial, dw_workspace};
    const SmxEdgeOperands o{ef, eperm, wt, bias, K, (K % 4 == 0 && aligned(ef, 16)) ? 1 : 0};
    const int vec = pick_vec(F, {ldx, ldd, ldo, ldl, a.lddx}, {x, dout, out, lse, dx, wt, bias});
    int64_t used = 0;
    if (dweight) dispatch_kp(SmxEdgeBwdLaunch<true>{a, o, dw_rows, &used, st}, K, F, vec);
    else dispatch_kp(SmxEdgeBwdLaunch<false>{a, o, dw_rows, &used, st}, K, F, vec);
    BOT_REQUIRE(used > 0, BOT_E_RANGE, "spmm_softmax_edge_bwd: dw_workspace holds %lld workgroup partials, the sweep needs %lld",
                (long long)dw_rows, (long long)-used);
    if (int rc = hip_status("spmm_softmax_edge_bwd launch")) return rc;
    if (dx && n_long > 0) {
        launch_sum_combine(partial, F, dx, lddx, long_rows, long_ptr, n_long, st);
        if (int rc = hip_status("spmm_softmax_edge_bwd combine launch")) return rc;
    }
    if (dweight) {
        hipLaunchKernelGGL(spmm_softmax_edge_dw_kernel, dim3((unsigned)(((int64_t)K * F + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, dw_workspace,
                           used, K, F, dweight);
        if (int rc = hip_status("spmm_softmax_edge_bwd dweight launch")) return rc;
    }
    return 0;
}

}  // extern "C"
