// Principal Neighbourhood Aggregation (Corso, Cavalleri, Beaini, Lio, Velickovic, NeurIPS 2020; include/bot_gnn.h "PNA aggregation") for
// gfx950: mean / sum / max / min / std / var of the same neighbourhood, each times scalers of the in-degree, in ONE gather of the source
// rows (bot_amd.nn.PNAConv, ops.pna_aggregate, `update_all(fn.copy_u, fn.min)`).
//   forward   per destination r with n in-edges at positions k, m_k = a[indices[k]] + b[r]:  the chosen aggregators of m, each times
//             scale[s, r], stored tower-major: column tower * S*A*Ft + (s*A + agg) * Ft + f                  (rows = destinations: the CSC)
//   prep      the dense pass of the backward: dout folded over the scalers into one packed record per destination, and db
//   backward  dx[u] = sum_j g0[v_j] + c1[v_j] * (a[u] - mean[v_j]) + gmax[v_j] * (argmax[v_j] == pos_j) + gmin[v_j] * (argmin[v_j] == pos_j)
//                                                                                                             (rows = sources: the CSR)
//
// The gather is the lane-group row sweep that sweep.h describes, the walk written out as in spmm_max.hip.  Per column a lane keeps
// S1 = sum d_k, S2 = sum d_k^2 and the running (max, position) and (min, position) pairs in registers, with d_k = a[u_k] - p and the
// PIVOT p = the row of the row's first neighbour: mean = p + S1 / n and var = relu(S2 / n - (S1 / n)^2) are then formed from numbers of
// the size of the spread, not of the mean - a constant row and a row of one neighbour give exactly var = 0, and a shift of `a` by 1000
// costs nothing - which the raw moments sum a_k^2 / n - mean^2 do not do in float32.  Every chunk of a long row uses the ROW's pivot, so
// the chunks' sums add plainly.  Max and min run on a itself with a strict compare in position order: the earliest position of a tie
// owns it, -0.0 == +0.0, a NaN never enters; b[r] is added behind the reduce (every aggregator commutes with the shift, std and var
// ignore it).  The chunks of a long row leave (S1, S2, max, pos, min, pos) in the workspace; spmm_pna_combine_kernel (one thread per long
// row and column) folds them in slot order (= position order) and runs the same epilogue.
//
// No atomics in any of the three: the bytes repeat from call to call.
//
// HBM model: forward 4 * [E * (1 + F) + n_rows * (S*A*F + F)] bytes (ids and source rows per edge; the output row and b per row; + 4 F
// words per row when the backward's saved arrays are written); backward 4 * [E * (2 + R) + 2 * n_src * F] with R the record's words
// (ids, positions and one record per edge; a[u] and dx per row).
#include "pna.h"

namespace bot {

template <int VEC, int LANES, int NCHUNK>
__global__ __launch_bounds__(kBlock) void spmm_pna_kernel(PnaArgs a) {
    constexpr int U = 4;
    constexpr int TILE = LANES * VEC * NCHUNK;
    const int lane = threadIdx.x % LANES;
    const int64_t item = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / LANES;
    if (item >= a.n_items) return;  // whole groups leave together
    const RowItem it = load_item<LANES>(a.items, item);
    const bool some = it.beg < it.end;
    const float* prow = some ? pna_pivot(a, it.slot >= 0 ? a.indptr[it.row] : it.beg) : a.a;
    for (int col0 = 0; col0 < a.F; col0 += TILE) {  // groups narrower than a wavefront have one tile (PnaLaunch)
        const ColTile<VEC, LANES, NCHUNK> tile(col0, lane, a.F);
        float pv[NCHUNK][VEC], s1[NCHUNK][VEC], s2[NCHUNK][VEC], mx[NCHUNK][VEC], mn[NCHUNK][VEC];
        int am[NCHUNK][VEC], an[NCHUNK][VEC];
#pragma unroll
        for (int c = 0; c < NCHUNK; ++c) {
            if (some) vload<VEC>(pv[c], prow + tile.off[c]);
#pragma unroll
            for (int t = 0; t < VEC; ++t) {
                if (!some) pv[c][t] = 0.f;
                s1[c][t] = s2[c][t] = 0.f;
                mx[c][t] = -INFINITY;
                mn[c][t] = INFINITY;
                am[c][t] = an[c][t] = some ? it.beg : -1;
            }
        }
        for (int k0 = it.beg; k0 < it.end; k0 += LANES) {
            const int k = k0 + lane;
            const int idx = k < it.end ? a.indices[k] : 0;
            const int cnt = min(LANES, it.end - k0);
            int i = 0;
            for (; i + U <= cnt; i += U) {
                float v[U][NCHUNK][VEC];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int s = group_bcast<LANES>(idx, i + u);
                    const float* p = a.a + (int64_t)s * a.lda;
#pragma unroll
                    for (int c = 0; c < NCHUNK; ++c) vload<VEC>(v[u][c], p + tile.off[c]);
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int c = 0; c < NCHUNK; ++c)
#pragma unroll
                        for (int t = 0; t < VEC; ++t) {
                            const float x = v[u][c][t], d = x - pv[c][t];
                            s1[c][t] += d;
                            s2[c][t] = fmaf(d, d, s2[c][t]);
                            if (x > mx[c][t]) {
                                mx[c][t] = x;
                                am[c][t] = k0 + i + u;
                            }
                            if (x < mn[c][t]) {
                                mn[c][t] = x;
                                an[c][t] = k0 + i + u;
                            }
                        }
            }
            for (; i < cnt; ++i) {
                const int s = group_bcast<LANES>(idx, i);
                const float* p = a.a + (int64_t)s * a.lda;
                float v[NCHUNK][VEC];
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c) vload<VEC>(v[c], p + tile.off[c]);
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c)
#pragma unroll
                    for (int t = 0; t < VEC; ++t) {
                        const float x = v[c][t], d = x - pv[c][t];
                        s1[c][t] += d;
                        s2[c][t] = fmaf(d, d, s2[c][t]);
                        if (x > mx[c][t]) {
                            mx[c][t] = x;
                            am[c][t] = k0 + i;
                        }
                        if (x < mn[c][t]) {
                            mn[c][t] = x;
                            an[c][t] = k0 + i;
                        }
                    }
            }
        }
        if (it.slot >= 0) {  // a chunk of a long row: the raw accumulators, folded by spmm_pna_combine_kernel
            float* w = a.ws + (int64_t)it.slot * a.F;
#pragma unroll
            for (int c = 0; c < NCHUNK; ++c)
                if (tile.act[c]) {
                    vstore<VEC>(w + tile.off[c], s1[c]);
                    vstore<VEC>(w + a.plane + tile.off[c], s2[c]);
                    vstore<VEC>(w + 2 * a.plane + tile.off[c], mx[c]);
                    ivstore_pna<VEC>(reinterpret_cast<int32_t*>(w + 3 * a.plane) + tile.off[c], am[c]);
                    vstore<VEC>(w + 4 * a.plane + tile.off[c], mn[c]);
                    ivstore_pna<VEC>(reinterpret_cast<int32_t*>(w + 5 * a.plane) + tile.off[c], an[c]);
                }
            continue;
        }
#pragma unroll
        for (int c = 0; c < NCHUNK; ++c)
            if (tile.act[c]) pna_finish<VEC>(a, it.row, tile.off[c], it.end - it.beg, pv[c], s1[c], s2[c], mx[c], am[c], mn[c], an[c]);
    }
}

// One thread per (long row, column): the chunks' accumulators are folded in slot order (= position order) - the sums add plainly, every
// chunk having used the row's pivot, the pairs with the sweep's strict compares, the first chunk's taken as they are - then the row's
// epilogue.
__global__ __launch_bounds__(kBlock) void spmm_pna_combine_kernel(PnaArgs a, const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long) {
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
        const int64_t o = (int64_t)s * a.F + c;
        mx[0] = a.ws[o + 2 * a.plane];
        am[0] = wi[o + 3 * a.plane];
        mn[0] = a.ws[o + 4 * a.plane];
        an[0] = wi[o + 5 * a.plane];
    }
    for (; s < p1; ++s) {
        const int64_t o = (int64_t)s * a.F + c;
        s1[0] += a.ws[o];
        s2[0] += a.ws[o + a.plane];
        const float v = a.ws[o + 2 * a.plane], w = a.ws[o + 4 * a.plane];
        if (v > mx[0]) {
            mx[0] = v;
            am[0] = wi[o + 3 * a.plane];
        }
        if (w < mn[0]) {
            mn[0] = w;
            an[0] = wi[o + 5 * a.plane];
        }
    }
    if (n > 0) p[0] = pna_pivot(a, first)[c];
    pna_finish<1>(a, row, c, n, p, s1, s2, mx, am, mn, an);
}

struct PnaLaunch {
    const PnaArgs& a;
    hipStream_t st;
    template <int VEC, int LANES, int NCHUNK>
    void run() const {
        const int64_t blocks = (a.n_items * LANES + kBlock - 1) / kBlock;
        if (blocks == 0) return;
        set_kernel("bot::spmm_pna_kernel<%d,%d,%d>", VEC, LANES, NCHUNK);
        hipLaunchKernelGGL((spmm_pna_kernel<VEC, LANES, NCHUNK>), dim3((unsigned)blocks), dim3(kBlock), 0, st, a);
    }
    template <int VEC>
    void wide(int) const {
        run<VEC, 64, 2>();  // wider rows walk tiles of 128 lanes
    }
};

// ---------------------------------------------------------------------------------------------- backward
struct PnaPrepArgs {
    const int32_t* indptr;
    int64_t n_rows;
    const float* dout;
    int64_t ldd;
    const float* scale;
    int32_t F, Ft, A, S;
    int8_t code[kPnaMax];
    const float* saved;
    int64_t lds;
    const int32_t* sarg;
    int64_t ldg;
    float* db;  // may be NULL
    int64_t ldb;
    float* rec;
    int64_t ldr;
    int32_t off[kSecs];  // the first word of each section of a record, -1: not in it
};

// One thread per (destination, column): dout folded over the scalers, per aggregator; the record's sections; db.
__global__ __launch_bounds__(kBlock) void pna_bwd_prep_kernel(PnaPrepArgs a) {
    const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gid >= a.n_rows * a.F) return;
    const int64_t v = gid / a.F;
    const int f = (int)(gid - v * a.F);
    const int n = a.indptr[v + 1] - a.indptr[v];
    float g0 = 0.f, c1 = 0.f, gmax = 0.f, gmin = 0.f, db = 0.f, mu = 0.f;
    int amax = -1, amin = -1;
    if (n > 0) {
        const int t0 = f / a.Ft;
        const float* d = a.dout + v * a.ldd + (int64_t)t0 * a.S * a.A * a.Ft + (f - t0 * a.Ft);
        const float fn = (float)n;
        const float sd = a.saved[v * a.lds + a.F + f];
        mu = a.saved[v * a.lds + f];
        amax = a.sarg[v * a.ldg + f];
        amin = a.sarg[v * a.ldg + a.F + f];
        for (int g = 0; g < a.A; ++g) {
            float G = 0.f;
            for (int s = 0; s < a.S; ++s) G += (a.scale ? a.scale[(int64_t)s * a.n_rows + v] : 1.f) * d[(int64_t)(s * a.A + g) * a.Ft];
            switch (a.code[g]) {
                case kMean: g0 += G / fn; db += G; break;
                case kSum: g0 += G; db += fn * G; break;
                case kMax: gmax += G; db += G; break;
                case kMin: gmin += G; db += G; break;
                case kStd: c1 += sd > 0.f ? G / (fn * sd) : 0.f; break;
                default: c1 += sd > 0.f ? 2.f * G / fn : 0.f; break;
            }
        }
    }
    float* r = a.rec + v * a.ldr + f;
    if (a.off[kG0] >= 0) r[a.off[kG0]] = g0;
    if (a.off[kC1] >= 0) {
        r[a.off[kC1]] = c1;
        r[a.off[kMu]] = mu;
    }
    if (a.off[kGmax] >= 0) {
        r[a.off[kGmax]] = gmax;
        r[a.off[kAmax]] = __int_as_float(amax);
    }
    if (a.off[kGmin] >= 0) {
        r[a.off[kGmin]] = gmin;
        r[a.off[kAmin]] = __int_as_float(amin);
    }
    if (a.db) a.db[v * a.ldb + f] = db;
}

struct PnaBwdArgs {
    const int32_t* indices;
    const int32_t* pos;
    const int4* items;
    int64_t n_items;
    const float* a;
    int64_t lda;
    const float* rec;
    int64_t ldr;
    float* dx;
    int64_t ldx;
    int32_t F;
    float* partial;  // [n_slots, F] chunk sums
    int32_t off[kSecs];
};

template <int VEC, int LANES, int NCHUNK>
__global__ __launch_bounds__(kBlock) void spmm_pna_bwd_kernel(PnaBwdArgs a) {
    constexpr int U = 4;
    constexpr int TILE = LANES * VEC * NCHUNK;
    static_assert(NCHUNK == 1, "one chunk of columns per lane: up to seven record sections are staged per neighbour");
    const int lane = threadIdx.x % LANES;
    const int64_t item = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / LANES;
    if (item >= a.n_items) return;  // whole groups leave together
    const RowItem it = load_item<LANES>(a.items, item);
    const bool h0 = a.off[kG0] >= 0, h1 = a.off[kC1] >= 0, hx = a.off[kGmax] >= 0, hn = a.off[kGmin] >= 0;
    for (int col0 = 0; col0 < a.F; col0 += TILE) {
        const ColTile<VEC, LANES, 1> tile(col0, lane, a.F);
        const int off = tile.off[0];
        float acc[1][VEC] = {}, av[VEC] = {};
        if (h1) vload<VEC>(av, a.a + (int64_t)it.row * a.lda + off);
        for (int k0 = it.beg; k0 < it.end; k0 += LANES) {
            const int k = k0 + lane;
            int idx = 0, pk = -2;  // -2: no position equals it
            if (k < it.end) {
                idx = a.indices[k];
                pk = a.pos[k];
            }
            const int cnt = min(LANES, it.end - k0);
            for (int i = 0; i < cnt; i += U) {
                float g0[U][VEC] = {}, c1[U][VEC] = {}, mu[U][VEC] = {}, gx[U][VEC] = {}, gn[U][VEC] = {}, ax[U][VEC] = {}, an[U][VEC] = {};
                int pp[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    pp[u] = -2;
                    if (i + u < cnt) {  // uniform over the group
                        const int s = group_bcast<LANES>(idx, i + u);
                        pp[u] = group_bcast<LANES>(pk, i + u);
                        const float* r = a.rec + (int64_t)s * a.ldr + off;
                        if (h0) vload<VEC>(g0[u], r + a.off[kG0]);
                        if (h1) {
                            vload<VEC>(c1[u], r + a.off[kC1]);
                            vload<VEC>(mu[u], r + a.off[kMu]);
                        }
                        if (hx) {
                            vload<VEC>(gx[u], r + a.off[kGmax]);
                            vload<VEC>(ax[u], r + a.off[kAmax]);
                        }
                        if (hn) {
                            vload<VEC>(gn[u], r + a.off[kGmin]);
                            vload<VEC>(an[u], r + a.off[kAmin]);
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
                    if (i + u < cnt) {
#pragma unroll
                        for (int t = 0; t < VEC; ++t) {
                            float e = g0[u][t];
                            if (h1) e = fmaf(c1[u][t], av[t] - mu[u][t], e);
                            if (hx) e += __float_as_int(ax[u][t]) == pp[u] ? gx[u][t] : 0.f;
                            if (hn) e += __float_as_int(an[u][t]) == pp[u] ? gn[u][t] : 0.f;
                            acc[0][t] += e;
                        }
                    }
            }
        }
        tile.store(sum_row(it, a.dx, a.ldx, a.partial, a.F), acc);
    }
}

struct PnaBwdLaunch {
    const PnaBwdArgs& a;
    hipStream_t st;
    template <int VEC, int LANES, int NCHUNK>
    void run() const {
        const int64_t blocks = (a.n_items * LANES + kBlock - 1) / kBlock;
        if (blocks == 0) return;
        set_kernel("bot::spmm_pna_bwd_kernel<%d,%d,%d>", VEC, LANES, NCHUNK);
        hipLaunchKernelGGL((spmm_pna_bwd_kernel<VEC, LANES, NCHUNK>), dim3((unsigned)blocks), dim3(kBlock), 0, st, a);
    }
    template <int VEC>
    void wide(int) const {
        run<VEC, 64, 1>();  // wider rows walk tiles of 64 lanes
    }
};


}  // namespace bot

extern "C" {

int bot_spmm_pna_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                     const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots, const float* a, int64_t lda, const float* b,
                     int64_t ldb, int32_t F, int32_t Ft, const int32_t* aggs, int32_t A, const float* scale, int32_t S, int32_t pivot, float* out,
                     int64_t ldo, float* saved, int64_t lds, int32_t* sarg, int64_t ldg, void* workspace, bot_stream_t stream) {
    using namespace bot;
    if (int rc = check_plan_sizes("spmm_pna", n_rows, nnz, n_items, n_long, n_slots)) return rc;
    BOT_REQUIRE(F >= 1, BOT_E_RANGE, "spmm_pna: F=%d (>= 1)", F);
    BOT_REQUIRE(Ft >= 1 && F % Ft == 0, BOT_E_RANGE, "spmm_pna: the tower width Ft=%d does not divide F=%d", Ft, F);
    BOT_REQUIRE(S >= 1 && S <= kPnaMax, BOT_E_RANGE, "spmm_pna: S=%d scalers (1 .. %d)", S, kPnaMax);
    PnaArgs k{};
    int32_t off[kSecs];
    if (int rc = pna_codes("spmm_pna", aggs, A, F, k.code, off); rc < 0) return rc;
    if (n_rows == 0) return 0;
    if (int rc = check_plan("spmm_pna", items, "items/indptr/out", indptr && out, nnz, "indices/a", indices && a, n_long,
                            "long_rows/long_ptr/workspace", long_rows && long_ptr && workspace))
        return rc;
    BOT_REQUIRE((saved == nullptr) == (sarg == nullptr), BOT_E_NULL, "spmm_pna: saved and sarg come together");
    BOT_REQUIRE(S == 1 || scale, BOT_E_NULL, "spmm_pna: S=%d scalers without a scale table", S);
    BOT_REQUIRE(n_long == 0 || n_slots > 0, BOT_E_RANGE, "spmm_pna: long rows without slots");
    BOT_REQUIRE(out != a && out != b, BOT_E_RANGE, "spmm_pna: out aliases an operand");
    const int64_t W = (int64_t)S * A * F;
    BOT_REQUIRE(lda >= F && (!b || ldb >= F) && ldo >= W && (!saved || (lds >= 2 * (int64_t)F && ldg >= 2 * (int64_t)F)), BOT_E_RANGE,
                "spmm_pna: row strides smaller than the rows (F=%d, out %lld: lda=%lld ldb=%lld ldo=%lld lds=%lld ldg=%lld)", F, (long long)W,
                (long long)lda, (long long)ldb, (long long)ldo, (long long)lds, (long long)ldg);
    BOT_REQUIRE(aligned(a, 4) && aligned(b, 4) && aligned(out, 4) && aligned(saved, 4) && aligned(sarg, 4) && aligned(scale, 4) &&
                    aligned(items, 16) && aligned(workspace, 16),
                BOT_E_ALIGN, "spmm_pna: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    k.indptr = indptr, k.indices = indices, k.items = reinterpret_cast<const int4*>(items), k.n_items = n_items, k.n_rows = n_rows;
    k.a = a, k.lda = lda, k.b = b, k.ldb = ldb, k.F = F, k.Ft = Ft, k.A = A, k.S = S, k.pivot = pivot, k.scale = scale;
    k.out = out, k.ldo = ldo, k.saved = saved, k.lds = lds, k.sarg = sarg, k.ldg = ldg;
    k.ws = static_cast<float*>(workspace), k.plane = n_slots * F;
    // a vector never straddles a tower, a block of the output row or a plane of the workspace: Ft, and with it F and S*A*Ft, is a multiple
    const int vec = pick_vec(Ft, {lda, b ? ldb : 0, ldo, saved ? lds : 0, saved ? ldg : 0, (int64_t)F}, {a, b, out, saved, sarg});
    dispatch_sweep(PnaLaunch{k, st}, F, vec);
    if (int rc = hip_status("spmm_pna launch")) return rc;
    if (n_long > 0) {
        hipLaunchKernelGGL(spmm_pna_combine_kernel, dim3((unsigned)((n_long * F + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, k, long_rows,
                           long_ptr, n_long);
        if (int rc = hip_status("spmm_pna combine launch")) return rc;
    }
    return 0;
}

int bot_pna_bwd_prep_f32(const int32_t* indptr, int64_t n_rows, const float* dout, int64_t ldd, const float* scale, int32_t S, const int32_t* aggs,
                         int32_t A, int32_t F, int32_t Ft, const float* saved, int64_t lds, const int32_t* sarg, int64_t ldg, float* db, int64_t ldb,
                         float* rec, int64_t ldr, bot_stream_t stream) {
    using namespace bot;
    BOT_REQUIRE(n_rows >= 0 && n_rows < INT32_MAX, BOT_E_RANGE, "pna_bwd_prep: n_rows out of range");
    BOT_REQUIRE(F >= 1, BOT_E_RANGE, "pna_bwd_prep: F=%d (>= 1)", F);
    BOT_REQUIRE(Ft >= 1 && F % Ft == 0, BOT_E_RANGE, "pna_bwd_prep: the tower width Ft=%d does not divide F=%d", Ft, F);
    BOT_REQUIRE(S >= 1 && S <= kPnaMax, BOT_E_RANGE, "pna_bwd_prep: S=%d scalers (1 .. %d)", S, kPnaMax);
    PnaPrepArgs k{};
    const int nsec = pna_codes("pna_bwd_prep", aggs, A, F, k.code, k.off);
    if (nsec < 0) return nsec;
    if (n_rows == 0) return 0;
    BOT_REQUIRE(indptr && dout && saved && sarg && rec, BOT_E_NULL, "pna_bwd_prep: indptr/dout/saved/sarg/rec is NULL");
    BOT_REQUIRE(S == 1 || scale, BOT_E_NULL, "pna_bwd_prep: S=%d scalers without a scale table", S);
    BOT_REQUIRE(ldd >= (int64_t)S * A * F && lds >= 2 * (int64_t)F && ldg >= 2 * (int64_t)F && (!db || ldb >= F) && ldr >= (int64_t)nsec * F,
                BOT_E_RANGE, "pna_bwd_prep: row strides smaller than the rows (F=%d: ldd=%lld lds=%lld ldg=%lld ldb=%lld ldr=%lld)", F,
                (long long)ldd, (long long)lds, (long long)ldg, (long long)ldb, (long long)ldr);
    BOT_REQUIRE(aligned(dout, 4) && aligned(saved, 4) && aligned(sarg, 4) && aligned(db, 4) && aligned(rec, 4) && aligned(scale, 4), BOT_E_ALIGN,
                "pna_bwd_prep: misaligned pointer");
    k.indptr = indptr, k.n_rows = n_rows, k.dout = dout, k.ldd = ldd, k.scale = scale, k.F = F, k.Ft = Ft, k.A = A, k.S = S;
    k.saved = saved, k.lds = lds, k.sarg = sarg, k.ldg = ldg, k.db = db, k.ldb = ldb, k.rec = rec, k.ldr = ldr;
    set_kernel("bot::pna_bwd_prep_kernel");
    hipLaunchKernelGGL(pna_bwd_prep_kernel, dim3((unsigned)((n_rows * F + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)stream, k);
    return hip_status("pna_bwd_prep launch");
}

int bot_spmm_pna_bwd_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                         const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, const int32_t* pos, const float* a, int64_t lda,
                         const float* rec, int64_t ldr, const int32_t* aggs, int32_t A, int32_t F, float* dx, int64_t ldx, float* partial,
                         bot_stream_t stream) {
    using namespace bot;
    (void)indptr;
    if (int rc = check_plan_sizes("spmm_pna_bwd", n_rows, nnz, n_items, n_long)) return rc;
    BOT_REQUIRE(F >= 1, BOT_E_RANGE, "spmm_pna_bwd: F=%d (>= 1)", F);
    PnaBwdArgs k{};
    int8_t code[kPnaMax];
    const int nsec = pna_codes("spmm_pna_bwd", aggs, A, F, code, k.off);
    if (nsec < 0) return nsec;
    if (n_rows == 0) return 0;
    if (int rc = check_plan("spmm_pna_bwd", items, "items/dx", dx, nnz, "indices/pos/rec", indices && pos && rec, n_long,
                            "long_rows/long_ptr/partial", long_rows && long_ptr && partial))
        return rc;
    BOT_REQUIRE(k.off[kC1] < 0 || a, BOT_E_NULL, "spmm_pna_bwd: std / var need a");
    BOT_REQUIRE(ldx >= F && (!a || lda >= F) && ldr >= (int64_t)nsec * F, BOT_E_RANGE,
                "spmm_pna_bwd: row strides smaller than the rows (F=%d, record %lld: lda=%lld ldr=%lld ldx=%lld)", F, (long long)nsec * F,
                (long long)lda, (long long)ldr, (long long)ldx);
    BOT_REQUIRE(aligned(a, 4) && aligned(rec, 4) && aligned(dx, 4) && aligned(items, 16) && aligned(partial, 16), BOT_E_ALIGN,
                "spmm_pna_bwd: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    k.indices = indices, k.pos = pos, k.items = reinterpret_cast<const int4*>(items), k.n_items = n_items, k.a = a, k.lda = lda;
    k.rec = rec, k.ldr = ldr, k.dx = dx, k.ldx = ldx, k.F = F, k.partial = partial;
    const int vec = pick_vec(F, {a ? lda : 0, ldr, ldx}, {a, rec, dx});  // (the sections start at multiples of F)
    dispatch_sweep(PnaBwdLaunch{k, st}, F, vec);
    if (int rc = hip_status("spmm_pna_bwd launch")) return rc;
    if (n_long > 0) {
        launch_sum_combine(partial, F, dx, ldx, long_rows, long_ptr, n_long, st);
        if (int rc = hip_status("spmm_pna_bwd combine launch")) return rc;
    }
    return 0;
}

}  // extern "C"
