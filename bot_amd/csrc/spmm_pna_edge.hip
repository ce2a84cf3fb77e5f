// Principal Neighbourhood Aggregation with raw edge features (include/bot_gnn.h "PNA aggregation with edge features") for gfx950: DGL's
// PNAConv(edge_feat_size=K) pretrans M(cat[h_u, h_v, e_uv]) with the edge term formed inside the gather (bot_amd.nn.EdgePNAConv,
// `ops.pna_aggregate_edge`).  For an edge e = (u -> v) at position k of destination r:
//   c_k[f] = ef[e,0] wt[0,f], then fmaf(ef[e,j], wt[j,f], c) for j = 1 .. K-1     edge_term.h's chain: a rounded product, then K - 1 fmas
//   m_k    = a[u_k] + c_k                                                          b[r] enters behind the reduce, as in spmm_pna.hip
//   forward   the aggregators of spmm_pna.hip over the m_k of a destination's in-edges (rows = destinations: the CSC); max / min run on
//             m_k with the strict compares in position order
//   backward  dm_e = g0[v] + c1[v] * ((a[u] - mu[v]) + c_e) + gmax[v] * (argmax[v] == pos) + gmin[v] * (argmin[v] == pos), with the record
//             of bot_pna_bwd_prep_f32 (mu is now the messages' mean) and c_e formed again by the same chain;
//             da[u] = sum of dm_e over the out-edges of u;  dweight[f,j] = sum over all edges of ef[e,j] dm_e[f]   (rows = sources: the CSR)
// ef is [E, K] raw floats, K <= 16, read at row eperm[k] of position k (NULL: k itself): an edge streams 4 K bytes beside its 4 F-byte
// source row and no [E, F] message exists.  wt is the towers' edge columns transposed to [K, F]; a lane keeps its KP x VEC slice
// (KP = 4 / 8 / 16, zero padding) for the whole sweep.
//
// Moments: a SPLIT pivot.  p_a = a[u_0] and p_c = c_0 of the row's first position; d_k = (a_k - p_a) + (c_k - p_c), both differences of
// the size of the spread, so a shift of `a` by 1000 costs nothing, a row of constant messages gives var = 0 exactly, and constant ef
// across a row gives spmm_pna.hip's S1, S2 bit for bit.  P = p_a + p_c takes the place of the pivot in pna_finish (mean = P + S1 / n,
// sum = S1 + n P + n b).  Every chunk of a long row forms the ROW's pair again from the row's first position; the workspace keeps its
// six planes and spmm_pna_edge_combine_kernel folds them as spmm_pna_combine_kernel does.
//
// Forward: spmm_pna_kernel's registers and compares on sweep.h's walk_row, with the group-uniform load of the edge's K floats beside the
// source row (16-byte loads where K % 4 == 0 and ef is 16-byte aligned).  Rows wider than 64 lanes walk tiles of 64 lanes, so that one
// slice of wt is live.  Backward: one persistent sweep shaped like spmm_softmax_edge_bwd_kernel - feature tiles on grid.y, KP x VEC
// dweight partials per lane, added group by group through LDS in group order into dw_ws [grid.x, K, F], which
// spmm_pna_edge_dw_kernel adds in index order; grid.x is edge_bwd_blocks(n_items, lanes, tiles), never a function of the device.
// No atomics anywhere: two calls give the same bytes.
//
// HBM model: forward 4 * [E * (1 + K + F) + n * (S*A*F + F)] bytes (+ 4 E with an eperm; + 4 F words per row with the saved arrays);
// backward 4 * [E * (2 + K + R) + 2 * n_src * F] bytes (+ 4 E with an eperm) plus the partials, 4 * grid.x * K * F written and read
// once, with R the record's words.
#include "pna.h"

// Every product of the chain is rounded on its own and every fused multiply-add is written out (edge_term.h switches contraction off for
// the rest of this file), so the forward, its combine and the backward form the same c.  pna.h is included before it: the epilogue is
// spmm_pna.hip's arithmetic.
#include "edge_term.h"

namespace bot {

struct PnaEdgeOperands {
    const float* ef;       // [E, K]
    const int32_t* eperm;  // [nnz] the row of ef of a position, or NULL: the position
    const float* wt;       // [K, F]
    int32_t K;
    int32_t k4;            // ef rows are read with 16-byte loads
};

template <int KP, int VEC>
struct PnaEdgeStage {
    float v[VEC];
    float e[KP];
};

template <int KP, int VEC, int LANES>
__global__ __launch_bounds__(kBlock) void spmm_pna_edge_kernel(PnaArgs a, PnaEdgeOperands o) {
    constexpr int TILE = LANES * VEC;
    constexpr int U = KP > 8 ? 2 : 4;  // as in spmm_softmax_edge_kernel
    const int lane = threadIdx.x % LANES;
    const int64_t item = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / LANES;
    if (item >= a.n_items) return;  // whole groups leave together
    const RowItem it = load_item<LANES>(a.items, item);
    const bool some = it.beg < it.end;
    const int K = o.K;
    const bool k4 = o.k4 != 0;
    const int first = some ? (it.slot >= 0 ? a.indptr[it.row] : it.beg) : 0;  // the ROW's first position: every chunk uses its pair
    const float* prow = some ? a.a + (int64_t)a.indices[first] * a.lda : a.a;
    const float* pef = some ? o.ef + (int64_t)(o.eperm ? o.eperm[first] : first) * K : o.ef;
    for (int col0 = 0; col0 < a.F; col0 += TILE) {  // groups narrower than a wavefront have one tile
        const ColTile<VEC, LANES, 1> tile(col0, lane, a.F);
        const int off = tile.off[0];
        float w[KP][VEC], nob[VEC];
        load_slice<KP, VEC>(w, nob, o.wt, nullptr, K, a.F, off);
        float pa[VEC], pc[VEC], s1[VEC], s2[VEC], mx[VEC], mn[VEC];
        int am[VEC], an[VEC];
#pragma unroll
        for (int t = 0; t < VEC; ++t) {
            pa[t] = pc[t] = s1[t] = s2[t] = 0.f;
            mx[t] = -INFINITY;
            mn[t] = INFINITY;
            am[t] = an[t] = some ? it.beg : -1;
        }
        if (some) {
            float e0[KP];
            vload<VEC>(pa, prow + off);
            load_ef<KP>(e0, pef, K, k4);
#pragma unroll
            for (int t = 0; t < VEC; ++t) pc[t] = edge_chain<KP, VEC>(e0, w, t);
        }
        walk_row<LANES, PnaEdgeStage<KP, VEC>, U>(
            it.beg, it.end, lane, [&](int k, bool in) { return Edge{in ? a.indices[k] : 0, in ? (o.eperm ? o.eperm[k] : k) : 0}; },
            [&](int s, int r, PnaEdgeStage<KP, VEC>& g, int) {
                vload<VEC>(g.v, a.a + (int64_t)s * a.lda + off);
                load_ef<KP>(g.e, o.ef + (int64_t)r * K, K, k4);
            },
            [&](int, int, const PnaEdgeStage<KP, VEC>& g, int k) {
#pragma unroll
                for (int t = 0; t < VEC; ++t) {
                    const float c = edge_chain<KP, VEC>(g.e, w, t);
                    const float x = g.v[t] + c;
                    const float d = (g.v[t] - pa[t]) + (c - pc[t]);
                    s1[t] += d;
                    s2[t] = fmaf(d, d, s2[t]);
                    if (x > mx[t]) {
                        mx[t] = x;
                        am[t] = k;
                    }
                    if (x < mn[t]) {
                        mn[t] = x;
                        an[t] = k;
                    }
                }
            });
        if (!tile.act[0]) continue;
        if (it.slot >= 0) {  // a chunk of a long row: the raw accumulators, folded by spmm_pna_edge_combine_kernel
            float* ws = a.ws + (int64_t)it.slot * a.F;
            vstore<VEC>(ws + off, s1);
            vstore<VEC>(ws + a.plane + off, s2);
            vstore<VEC>(ws + 2 * a.plane + off, mx);
            ivstore_pna<VEC>(reinterpret_cast<int32_t*>(ws + 3 * a.plane) + off, am);
            vstore<VEC>(ws + 4 * a.plane + off, mn);
            ivstore_pna<VEC>(reinterpret_cast<int32_t*>(ws + 5 * a.plane) + off, an);
            continue;
        }
        float P[VEC];
#pragma unroll
        for (int t = 0; t < VEC; ++t) P[t] = pa[t] + pc[t];
        pna_finish<VEC>(a, it.row, off, it.end - it.beg, P, s1, s2, mx, am, mn, an);
    }
}

// One thread per (long row, column): spmm_pna_combine_kernel's fold in slot order, the pivot pair formed again from the row's first
// position by the sweep's chain (its padding adds +0 where K is below the instance's KP), then the row's epilogue.
__global__ __launch_bounds__(kBlock) void spmm_pna_edge_combine_kernel(PnaArgs a, PnaEdgeOperands o, const int32_t* long_rows, const int32_t* long_ptr,
                                                                       int64_t n_long) {
    const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gid >= n_long * a.F) return;
    const int64_t i = gid / a.F;
    const int c = (int)(gid - i * a.F);
    const int row = long_rows[i], p1 = long_ptr[i + 1];
    int s = long_ptr[i];
    const int first = a.indptr[row], n = a.indptr[row + 1] - first;
    float s1[1] = {0.f}, s2[1] = {0.f}, mx[1] = {-INFINITY}, mn[1] = {INFINITY}, p[1] = {0.f};
    int am[1] = {-1}, an[1] = {-1};
    const int32_t* wi = reinterpret_cast<const int32_t*>(a.ws);
    if (s < p1) {
        const int64_t w0 = (int64_t)s * a.F + c;
        mx[0] = a.ws[w0 + 2 * a.plane];
        am[0] = wi[w0 + 3 * a.plane];
        mn[0] = a.ws[w0 + 4 * a.plane];
        an[0] = wi[w0 + 5 * a.plane];
    }
    for (; s < p1; ++s) {
        const int64_t w0 = (int64_t)s * a.F + c;
        s1[0] += a.ws[w0];
        s2[0] += a.ws[w0 + a.plane];
        const float v = a.ws[w0 + 2 * a.plane], w = a.ws[w0 + 4 * a.plane];
        if (v > mx[0]) {
            mx[0] = v;
            am[0] = wi[w0 + 3 * a.plane];
        }
        if (w < mn[0]) {
            mn[0] = w;
            an[0] = wi[w0 + 5 * a.plane];
        }
    }
    if (n > 0) {
        const float* e = o.ef + (int64_t)(o.eperm ? o.eperm[first] : first) * o.K;
        float pc = e[0] * o.wt[c];
        for (int j = 1; j < o.K; ++j) pc = fmaf(e[j], o.wt[(int64_t)j * a.F + c], pc);
        if (o.K < edge_kp(o.K)) pc = fmaf(0.f, 0.f, pc);  // the padded chain's +0, where the sweep's instance pads
        p[0] = a.a[(int64_t)a.indices[first] * a.lda + c] + pc;
    }
    pna_finish<1>(a, row, c, n, p, s1, s2, mx, am, mn, an);
}

struct PnaEdgeLaunch {
    const PnaArgs& a;
    const PnaEdgeOperands& o;
    hipStream_t st;
    template <int KP>
    struct At {
        const PnaEdgeLaunch& l;
        template <int VEC, int LANES, int NCHUNK>
        void run() const {
            const int64_t blocks = (l.a.n_items * LANES + kBlock - 1) / kBlock;
            if (blocks == 0) return;
            set_kernel("bot::spmm_pna_edge_kernel<%d,%d,%d>", KP, VEC, LANES);
            hipLaunchKernelGGL((spmm_pna_edge_kernel<KP, VEC, LANES>), dim3((unsigned)blocks), dim3(kBlock), 0, l.st, l.a, l.o);
        }
        template <int VEC>
        void wide(int) const {
            run<VEC, 64, 1>();  // wider rows walk tiles of 64 lanes: one tile's slice of wt is live
        }
    };
};

// ---------------------------------------------------------------------------------------------- backward
struct PnaEdgeBwdArgs {
    const int32_t* indices;
    const int32_t* pos;
    const int4* items;
    int64_t n_items;
    const float* a;
    int64_t lda;
    const float* rec;
    int64_t ldr;
    float* dx;  // the instances with WX
    int64_t ldx;
    int32_t F;
    float* partial;  // [n_slots, F] chunk sums of dx
    float* dw_ws;    // [gridDim.x, K, F] the workgroups' partials of dweight (the instances with WD)
    int32_t off[kSecs];
};

template <int KP, int VEC>
struct PnaEdgeBwdStage {
    float g0[VEC], c1[VEC], mu[VEC], gx[VEC], gn[VEC], ax[VEC], an[VEC];
    float e[KP];
    int pp;
};

template <bool WX, bool WD, int KP, int VEC, int LANES>
__global__ __launch_bounds__(kBlock) void spmm_pna_edge_bwd_kernel(PnaEdgeBwdArgs a, PnaEdgeOperands o) {
    constexpr int TILE = LANES * VEC, G = kBlock / LANES;
    constexpr int U = KP > 8 ? 1 : 2;  // up to seven record sections and the ef row are staged per neighbour
    __shared__ float red[WD ? kBlock * VEC : 1];
    const int lane = threadIdx.x % LANES, grp = threadIdx.x / LANES;
    const int K = o.K;
    const bool k4 = o.k4 != 0;
    const bool h0 = a.off[kG0] >= 0, h1 = a.off[kC1] >= 0, hx = a.off[kGmax] >= 0, hn = a.off[kGmin] >= 0;
    const ColTile<VEC, LANES, 1> tile((int)blockIdx.y * TILE, lane, a.F);
    const int off = tile.off[0];
    float w[KP][VEC], nob[VEC], dw[WD ? KP : 1][VEC] = {};
    load_slice<KP, VEC>(w, nob, o.wt, nullptr, K, a.F, off);
    // no thread leaves before the end: the fold below is a workgroup's
    for (int64_t item = (int64_t)blockIdx.x * G + grp; item < a.n_items; item += (int64_t)gridDim.x * G) {
        const RowItem it = load_item<LANES>(a.items, item);
        float av[VEC] = {}, acc[1][VEC] = {};
        if (h1) vload<VEC>(av, a.a + (int64_t)it.row * a.lda + off);
        for (int k0 = it.beg; k0 < it.end; k0 += LANES) {
            const int k = k0 + lane;
            int idx = 0, pk = -2, er = 0;  // -2: no position equals it
            if (k < it.end) {
                idx = a.indices[k];
                pk = a.pos[k];
                er = o.eperm ? o.eperm[k] : k;
            }
            const int cnt = min(LANES, it.end - k0);
            for (int i = 0; i < cnt; i += U) {
                PnaEdgeBwdStage<KP, VEC> g[U] = {};
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    g[u].pp = -2;
                    if (i + u < cnt) {  // uniform over the group
                        const int s = group_bcast<LANES>(idx, i + u);
                        const int r = group_bcast<LANES>(er, i + u);
                        g[u].pp = group_bcast<LANES>(pk, i + u);
                        const float* q = a.rec + (int64_t)s * a.ldr + off;
                        if (h0) vload<VEC>(g[u].g0, q + a.off[kG0]);
                        if (h1) {
                            vload<VEC>(g[u].c1, q + a.off[kC1]);
                            vload<VEC>(g[u].mu, q + a.off[kMu]);
                        }
                        if (hx) {
                            vload<VEC>(g[u].gx, q + a.off[kGmax]);
                            vload<VEC>(g[u].ax, q + a.off[kAmax]);
                        }
                        if (hn) {
                            vload<VEC>(g[u].gn, q + a.off[kGmin]);
                            vload<VEC>(g[u].an, q + a.off[kAmin]);
                        }
                        load_ef<KP>(g[u].e, o.ef + (int64_t)r * K, K, k4);
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (i + u < cnt) {
#pragma unroll
                        for (int t = 0; t < VEC; ++t) {
                            float e = g[u].g0[t];
                            if (h1) e = fmaf(g[u].c1[t], (av[t] - g[u].mu[t]) + edge_chain<KP, VEC>(g[u].e, w, t), e);
                            if (hx) e += __float_as_int(g[u].ax[t]) == g[u].pp ? g[u].gx[t] : 0.f;
                            if (hn) e += __float_as_int(g[u].an[t]) == g[u].pp ? g[u].gn[t] : 0.f;
                            acc[0][t] += e;
                            if constexpr (WD) {
#pragma unroll
                                for (int j = 0; j < KP; ++j) dw[j][t] = fmaf(g[u].e[j], e, dw[j][t]);
                            }
                        }
                    }
            }
        }
        if constexpr (WX) tile.store(sum_row(it, a.dx, a.ldx, a.partial, a.F), acc);
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
                    vstore<VEC>(a.dw_ws + ((int64_t)blockIdx.x * K + j) * a.F + off, s);
                }
                __syncthreads();
            }
    }
}

// dweight[f, j] = dw_ws[0, j, f] + dw_ws[1, j, f] + ... in workgroup order; one thread per (j, f)
__global__ __launch_bounds__(kBlock) void spmm_pna_edge_dw_kernel(const float* ws, int64_t n_blocks, int32_t K, int32_t F, float* dweight) {
    const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gid >= (int64_t)K * F) return;
    const int j = (int)(gid / F), f = (int)(gid - (int64_t)j * F);
    float s = 0.f;
    for (int64_t i = 0; i < n_blocks; ++i) s += ws[(i * K + j) * F + f];
    dweight[(int64_t)f * K + j] = s;
}

template <bool WX, bool WD>
struct PnaEdgeBwdLaunch {
    const PnaEdgeBwdArgs& a;
    const PnaEdgeOperands& o;
    int64_t dw_rows;  // the workgroup partials dw_ws holds
    int64_t* used;    // grid.x of the launch, negative when the workspace is too small
    hipStream_t st;
    template <int KP>
    struct At {
        const PnaEdgeBwdLaunch& l;
        template <int VEC, int LANES, int NCHUNK>
        void run() const {
            const int64_t n_tiles = (l.a.F + LANES * VEC - 1) / (LANES * VEC);
            const int64_t bx = edge_bwd_blocks(l.a.n_items, LANES, n_tiles);
            if (WD && bx > l.dw_rows) {
                *l.used = -bx;
                return;
            }
            *l.used = bx;
            set_kernel(WD ? (WX ? "bot::spmm_pna_edge_bwd_kernel<dx,dw,%d,%d,%d>" : "bot::spmm_pna_edge_bwd_kernel<dw,%d,%d,%d>")
                          : "bot::spmm_pna_edge_bwd_kernel<dx,%d,%d,%d>",
                       KP, VEC, LANES);
            hipLaunchKernelGGL((spmm_pna_edge_bwd_kernel<WX, WD, KP, VEC, LANES>), dim3((unsigned)bx, (unsigned)n_tiles), dim3(kBlock), 0, l.st,
                               l.a, l.o);
        }
        template <int VEC>
        void wide(int) const {
            run<VEC, 64, 1>();
        }
    };
};

static int check_pna_edge_operands(const char* who, int64_t nnz, const float* ef, int32_t K, const int32_t* eperm, const float* wt) {
    BOT_REQUIRE(K >= 1 && K <= kEdgeMaxK, BOT_E_RANGE, "%s: K=%d (1 .. %d)", who, K, kEdgeMaxK);
    BOT_REQUIRE(wt && (nnz == 0 || ef), BOT_E_NULL, "%s: ef/wt is NULL", who);
    BOT_REQUIRE(aligned(ef, 4) && aligned(wt, 4) && aligned(eperm, 4), BOT_E_ALIGN, "%s: misaligned pointer", who);
    return 0;
}

}  // namespace bot

extern "C" {

int bot_spmm_pna_edge_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                          const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots, const float* a, int64_t lda,
                          const float* b, int64_t ldb, int32_t F, int32_t Ft, const float* ef, int32_t K, const int32_t* eperm, const float* wt,
                          const int32_t* aggs, int32_t A, const float* scale, int32_t S, float* out, int64_t ldo, float* saved, int64_t lds,
                          int32_t* sarg, int64_t ldg, void* workspace, bot_stream_t stream) {
    using namespace bot;
    if (int rc = check_plan_sizes("spmm_pna_edge", n_rows, nnz, n_items, n_long, n_slots)) return rc;
    BOT_REQUIRE(F >= 1, BOT_E_RANGE, "spmm_pna_edge: F=%d (>= 1)", F);
    BOT_REQUIRE(Ft >= 1 && F % Ft == 0, BOT_E_RANGE, "spmm_pna_edge: the tower width Ft=%d does not divide F=%d", Ft, F);
    BOT_REQUIRE(S >= 1 && S <= kPnaMax, BOT_E_RANGE, "spmm_pna_edge: S=%d scalers (1 .. %d)", S, kPnaMax);
    PnaArgs k{};
    int32_t off[kSecs];
    if (int rc = pna_codes("spmm_pna_edge", aggs, A, F, k.code, off); rc < 0) return rc;
    if (int rc = check_pna_edge_operands("spmm_pna_edge", nnz, ef, K, eperm, wt)) return rc;
    if (n_rows == 0) return 0;
    if (int rc = check_plan("spmm_pna_edge", items, "items/indptr/out", indptr && out, nnz, "indices/a", indices && a, n_long,
                            "long_rows/long_ptr/workspace", long_rows && long_ptr && workspace))
        return rc;
    BOT_REQUIRE((saved == nullptr) == (sarg == nullptr), BOT_E_NULL, "spmm_pna_edge: saved and sarg come together");
    BOT_REQUIRE(S == 1 || scale, BOT_E_NULL, "spmm_pna_edge: S=%d scalers without a scale table", S);
    BOT_REQUIRE(n_long == 0 || n_slots > 0, BOT_E_RANGE, "spmm_pna_edge: long rows without slots");
    BOT_REQUIRE(out != a && out != b && out != ef && out != wt, BOT_E_RANGE, "spmm_pna_edge: out aliases an operand");
    const int64_t W = (int64_t)S * A * F;
    BOT_REQUIRE(lda >= F && (!b || ldb >= F) && ldo >= W && (!saved || (lds >= 2 * (int64_t)F && ldg >= 2 * (int64_t)F)), BOT_E_RANGE,
                "spmm_pna_edge: row strides smaller than the rows (F=%d, out %lld: lda=%lld ldb=%lld ldo=%lld lds=%lld ldg=%lld)", F, (long long)W,
                (long long)lda, (long long)ldb, (long long)ldo, (long long)lds, (long long)ldg);
    BOT_REQUIRE(aligned(a, 4) && aligned(b, 4) && aligned(out, 4) && aligned(saved, 4) && aligned(sarg, 4) && aligned(scale, 4) &&
                    aligned(items, 16) && aligned(workspace, 16),
                BOT_E_ALIGN, "spmm_pna_edge: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    k.indptr = indptr, k.indices = indices, k.items = reinterpret_cast<const int4*>(items), k.n_items = n_items, k.n_rows = n_rows;
    k.a = a, k.lda = lda, k.b = b, k.ldb = ldb, k.F = F, k.Ft = Ft, k.A = A, k.S = S, k.pivot = 1, k.scale = scale;
    k.out = out, k.ldo = ldo, k.saved = saved, k.lds = lds, k.sarg = sarg, k.ldg = ldg;
    k.ws = static_cast<float*>(workspace), k.plane = n_slots * F;
    const PnaEdgeOperands o{ef, eperm, wt, K, (K % 4 == 0 && aligned(ef, 16)) ? 1 : 0};
    // a vector never straddles a tower, a block of the output row, a plane of the workspace or a row of wt
    const int vec = pick_vec(Ft, {lda, b ? ldb : 0, ldo, saved ? lds : 0, saved ? ldg : 0, (int64_t)F}, {a, b, out, saved, sarg, wt});
    dispatch_kp(PnaEdgeLaunch{k, o, st}, K, F, vec);
    if (int rc = hip_status("spmm_pna_edge launch")) return rc;
    if (n_long > 0) {
        hipLaunchKernelGGL(spmm_pna_edge_combine_kernel, dim3((unsigned)((n_long * F + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, k, o, long_rows,
                           long_ptr, n_long);
        if (int rc = hip_status("spmm_pna_edge combine launch")) return rc;
    }
    return 0;
}

int bot_spmm_pna_edge_bwd_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                              const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, const int32_t* pos, const float* a, int64_t lda,
                              const float* ef, int32_t K, const int32_t* eperm, const float* wt, const float* rec, int64_t ldr,
                              const int32_t* aggs, int32_t A, int32_t F, float* dx, int64_t ldx, float* partial, float* dweight,
                              float* dw_workspace, int64_t dw_rows, bot_stream_t stream) {
    using namespace bot;
    (void)indptr;
    if (int rc = check_plan_sizes("spmm_pna_edge_bwd", n_rows, nnz, n_items, n_long)) return rc;
    BOT_REQUIRE(F >= 1, BOT_E_RANGE, "spmm_pna_edge_bwd: F=%d (>= 1)", F);
    BOT_REQUIRE(dw_rows >= 0, BOT_E_RANGE, "spmm_pna_edge_bwd: negative size");
    PnaEdgeBwdArgs k{};
    int8_t code[kPnaMax];
    const int nsec = pna_codes("spmm_pna_edge_bwd", aggs, A, F, code, k.off);
    if (nsec < 0) return nsec;
    if (int rc = check_pna_edge_operands("spmm_pna_edge_bwd", nnz, ef, K, eperm, wt)) return rc;
    if (!dx && !dweight) return 0;
    hipStream_t st = (hipStream_t)stream;
    BOT_REQUIRE(aligned(dweight, 4), BOT_E_ALIGN, "spmm_pna_edge_bwd: misaligned pointer");
    if (n_rows == 0) {  // no edge: dweight is zero, dx has no rows
        if (dweight) {
            (void)hipMemsetAsync(dweight, 0, sizeof(float) * (size_t)K * (size_t)F, st);
            if (int rc = hip_status("spmm_pna_edge_bwd memset")) return rc;
        }
        return 0;
    }
    if (int rc = check_plan("spmm_pna_edge_bwd", items, "items", true, nnz, "indices/pos/rec", indices && pos && rec, dx ? n_long : 0,
                            "long_rows/long_ptr/partial", long_rows && long_ptr && partial))
        return rc;
    BOT_REQUIRE(k.off[kC1] < 0 || a, BOT_E_NULL, "spmm_pna_edge_bwd: std / var need a");
    BOT_REQUIRE(!dweight || dw_workspace, BOT_E_NULL, "spmm_pna_edge_bwd: dweight needs dw_workspace");
    BOT_REQUIRE(!dx || (dx != a && dx != rec), BOT_E_RANGE, "spmm_pna_edge_bwd: dx aliases an input");
    BOT_REQUIRE((!dx || ldx >= F) && (!a || lda >= F) && ldr >= (int64_t)nsec * F, BOT_E_RANGE,
                "spmm_pna_edge_bwd: row strides smaller than the rows (F=%d, record %lld: lda=%lld ldr=%lld ldx=%lld)", F, (long long)nsec * F,
                (long long)lda, (long long)ldr, (long long)ldx);
    BOT_REQUIRE(aligned(a, 4) && aligned(rec, 4) && aligned(dx, 4) && aligned(pos, 4) && aligned(items, 16) && aligned(partial, 16) &&
                    aligned(dw_workspace, 16),
                BOT_E_ALIGN, "spmm_pna_edge_bwd: misaligned pointer");
    k.indices = indices, k.pos = pos, k.items = reinterpret_cast<const int4*>(items), k.n_items = n_items, k.a = a, k.lda = lda;
    k.rec = rec, k.ldr = ldr, k.dx = dx, k.ldx = dx ? ldx : F, k.F = F, k.partial = partial, k.dw_ws = dw_workspace;
    const PnaEdgeOperands o{ef, eperm, wt, K, (K % 4 == 0 && aligned(ef, 16)) ? 1 : 0};
    const int vec = pick_vec(F, {a ? lda : 0, ldr, k.ldx}, {a, rec, dx, wt});  // (the sections start at multiples of F)
    int64_t used = 0;
    if (dx && dweight) dispatch_kp(PnaEdgeBwdLaunch<true, true>{k, o, dw_rows, &used, st}, K, F, vec);
    else if (dx) dispatch_kp(PnaEdgeBwdLaunch<true, false>{k, o, dw_rows, &used, st}, K, F, vec);
    else dispatch_kp(PnaEdgeBwdLaunch<false, true>{k, o, dw_rows, &used, st}, K, F, vec);
    BOT_REQUIRE(used > 0, BOT_E_RANGE, "spmm_pna_edge_bwd: dw_workspace holds %lld workgroup partials, the sweep needs %lld", (long long)dw_rows,
                (long long)-used);
    if (int rc = hip_status("spmm_pna_edge_bwd launch")) return rc;
    if (dx && n_long > 0) {
        launch_sum_combine(partial, F, dx, ldx, long_rows, long_ptr, n_long, st);
        if (int rc = hip_status("spmm_pna_edge_bwd combine launch")) return rc;
    }
    if (dweight) {
        hipLaunchKernelGGL(spmm_pna_edge_dw_kernel, dim3((unsigned)(((int64_t)K * F + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, dw_workspace, used,
                           K, F, dweight);
        if (int rc = hip_status("spmm_pna_edge_bwd dweight launch")) return rc;
    }
    return 0;
}

}  // extern "C"
