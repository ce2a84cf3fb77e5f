// Dot-product attention with K raw edge features in the key and the value (include/bot_gnn.h "Dot-product attention with edge
// features") for gfx950: PyG's TransformerConv(edge_dim=K), the layer of UniMP on graphs with edge features (bot_amd.nn
// EdgeTransformerConv, `ops.dot_attention_edge`).  With E_e = W ef_e the edge encoder's row of the in-edge e = u -> v and W viewed as
// [H, D, K], PyG's layer is s_e = scale <q[v,h], k[u,h] + E_e[h]>, out[v,h] = sum_e p_e (v[u,h] + E_e[h]).  Everything the edge term
// touches is linear, so the encoder stays OUTSIDE the sweep:
//   <q[v,h], E_e[h]> = <qe[v,h], ef_e>       qe[v,h,:]  = q[v,h,:] W[h]      a dense product before the sweep
//   sum_e p_e E_e[h] = W[h] aef[v,h,:]       aef[v,h,:] = sum_e p_e ef_e     reduced here, projected after the sweep
// The sweeps carry K raw floats per edge and K accumulators per head; the weights never enter a kernel.
//   forward        s_k = scale (<q[v,h], k[u_k,h]> + <qe[v,h], ef_k>),  lse, a_k as in dot_attn.hip,
//                  out[v,h,:] = c sum_k keep_k a_k v[u_k,h,:],  aef[v,h,:] = c sum_k keep_k a_k ef_k
//   backward, dst  delta[v,h] = <dout[v,h], out[v,h]> + <daef[v,h], aef[v,h]>,  dd_k = <dout[v,h], v[u_k,h]> + <daef[v,h], ef_k>,
//                  p_k = c keep_k a_k,  ds_k = a_k (c keep_k dd_k - delta[v,h]),  dq[v,h,:] = scale sum_k ds_k k[u_k,h,:],
//                  dqe[v,h,:] = scale sum_k ds_k ef_k;  stores p[k,h], ds[k,h]
// dk and dv depend only on the stored p and ds: the backward over the sources is dot_attn.hip's, unchanged.
//
// Both kernels are dot_attn.hip's (non-shared form) with the edge term laid over the same lanes: the j-th vector slot of a head,
// (column - h D) / VEC == j < K, OWNS edge column j - one qe word, one staged ef word per neighbour in flight and one accumulator.  The
// ef row of a position is one coalesced read of K words by the owning lanes of every head; ef is in POSITION order, so the walk hands
// the position to the fetch (sweep.h walk_row_at) and the edge word stays the keep mask.  The owner's product qe ef joins the lane's partial
// logit BEFORE the head reduction (HeadTile::total), so the order of the sum is fixed per instance and there is still one exponential per
// lane, chunk and neighbour.  Every column needs an owner: D / VEC >= K, and the entry points narrow VEC until that holds.
//
// HBM model (4-byte words; HD = H*D, HK = H*K): forward 4 [E (1 + 2 HD + K) + n_dst (2 HD + H + 2 HK)]; backward over destinations
// 4 [E (1 + 2 HD + K + 2 H) + n_dst (4 HD + 2 H + 4 HK)] (the keep word adds E to each).
#include "dot.h"

#include <cmath>
#include <initializer_list>

namespace bot {

constexpr int kDotEdgeMaxK = 16;  // the widest raw edge feature (include/bot_gnn.h)

struct DotEdgeFwdArgs : DotPlan {
    const int32_t* keep;  // NULL: every edge kept
    float c;
    const float* q;
    int64_t ldq;
    const float* k;
    int64_t ldk;
    const float* v;
    int64_t ldv;
    const float* qe;  // [n_dst, H K]
    int64_t ldqe;
    const float* ef;  // [E, K], position order
    int64_t ldef;
    int32_t K, HK;
    float* out;
    int64_t ldo;
    float* lse;
    int64_t ldl;
    float* aef;  // [n_dst, H K]
    int64_t ldae;
    float* ws;  // S [n_slots, HD], M [n_slots, H], Z [n_slots, H], S_ef [n_slots, HK]: the chunks' states of the long rows
    int64_t n_slots;
};

struct DotEdgeDstArgs : DotPlan {
    const int32_t* keep;
    float c;
    const float* q;
    int64_t ldq;
    const float* k;
    int64_t ldk;
    const float* v;
    int64_t ldv;
    const float* qe;
    int64_t ldqe;
    const float* ef;
    int64_t ldef;
    int32_t K, HK;
    const float* dout;
    int64_t ldd;
    const float* out;
    int64_t ldo;
    const float* lse;
    int64_t ldl;
    const float* aef;
    int64_t ldae;
    const float* daef;
    int64_t lddae;
    float* pw;  // [E, H] p and ds, written
    float* ds;
    float* dq;  // NULL: not asked for
    int64_t lddq;
    float* dqe;  // NULL: not asked for
    int64_t lddqe;
    float* partial;  // dq [n_slots, HD], then dqe [n_slots, HK]: chunk sums of the long rows
    int64_t n_slots;
};

template <int VEC, int NCHUNK>
struct DotEdgeStage {
    float k[NCHUNK][VEC], v[NCHUNK][VEC], e[NCHUNK];  // e: the owner's word of the position's ef row, 0 elsewhere
};

// Neighbour rows in flight: dot_attn.hip's count for the same shape (the staged ef word is one register per chunk beside 2 VEC)
template <int VEC, int NCHUNK>
constexpr int dot_edge_unroll() {
    return dot_unroll(NCHUNK * VEC * 2);
}

// The edge column each of a lane's slots owns, or -1
template <int VEC, int LANES, int NCHUNK>
__device__ __forceinline__ void dot_edge_owner(const HeadTile<VEC, LANES, NCHUNK>& ht, int D, int K, int (&ej)[NCHUNK]) {
#pragma unroll
    for (int c = 0; c < NCHUNK; ++c) {
        const int j = (ht.off[c] - ht.head(c) * D) / VEC;
        ej[c] = ht.act[c] && j < K ? j : -1;
    }
}

template <int VEC, int LANES, int NCHUNK>
__global__ __launch_bounds__(kBlock) void dot_attn_edge_kernel(DotEdgeFwdArgs a) {
    using Stage = DotEdgeStage<VEC, NCHUNK>;
    constexpr int U = dot_edge_unroll<VEC, NCHUNK>();
    const int lane = threadIdx.x % LANES;
    const int64_t item = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / LANES;
    if (item >= a.n_items) return;  // whole groups leave together
    const RowItem it = load_item<LANES>(a.items, item);
    const int tcols = a.hpt * a.D;
    for (int col0 = 0; col0 < a.HD; col0 += tcols) {  // groups narrower than a wavefront have one tile (DotLaunch)
        const HeadTile<VEC, LANES, NCHUNK> ht(col0, min(a.HD, col0 + tcols), lane, a.D);
        float qv[NCHUNK][VEC], qe[NCHUNK], M[NCHUNK] = {}, Z[NCHUNK] = {}, S[NCHUNK][VEC] = {}, Se[NCHUNK] = {};
        int ej[NCHUNK];
        dot_edge_owner(ht, a.D, a.K, ej);
#pragma unroll
        for (int c = 0; c < NCHUNK; ++c) {
            vload<VEC>(qv[c], a.q + (int64_t)it.row * a.ldq + ht.off[c]);
            qe[c] = ej[c] >= 0 ? a.qe[(int64_t)it.row * a.ldqe + ht.hid[c] * a.K + ej[c]] : 0.f;
        }
        walk_row_at<LANES, Stage, U>(
            it.beg, it.end, lane, [&](int k, bool in) { return Edge{in ? a.indices[k] : 0, in && a.keep ? a.keep[k] : -1}; },
            [&](int s, int, Stage& st, int k) {
                const float* pk = a.k + (int64_t)s * a.ldk;
                const float* pv = a.v + (int64_t)s * a.ldv;
                const float* pe = a.ef + (int64_t)k * a.ldef;
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c) {
                    vload<VEC>(st.k[c], pk + ht.off[c]);
                    vload<VEC>(st.v[c], pv + ht.off[c]);
                    st.e[c] = ej[c] >= 0 ? pe[ej[c]] : 0.f;
                }
            },
            [&](int, int w, const Stage& st, int k) {
                float p[1][NCHUNK];
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c) {
                    p[0][c] = qv[c][0] * st.k[c][0];
#pragma unroll
                    for (int t = 1; t < VEC; ++t) p[0][c] += qv[c][t] * st.k[c][t];
                    p[0][c] = ej[c] >= 0 ? p[0][c] + qe[c] * st.e[c] : p[0][c];  // the edge term: before the head reduction
                }
                ht.template total<1>(p);
                if (k == it.beg) {  // the first neighbour is the state
#pragma unroll
                    for (int c = 0; c < NCHUNK; ++c) {
                        const bool kept = dot_kept(w, ht.hid[c]);
                        M[c] = a.scale * p[0][c];
                        Z[c] = 1.f;
#pragma unroll
                        for (int t = 0; t < VEC; ++t) S[c][t] = kept ? st.v[c][t] : 0.f;
                        Se[c] = kept ? st.e[c] : 0.f;
                    }
                    return;
                }
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c) {  // dot_attn_kernel's merge, with S_ef beside S
                    const bool kept = dot_kept(w, ht.hid[c]);
                    const float s = a.scale * p[0][c];
                    const float d = s - M[c];
                    const float e = smx_exp(-fabsf(d));
                    const bool up = d > 0.f;
                    const float fo = up ? e : 1.f, fn = up ? 1.f : e;
                    Z[c] = fmaf(Z[c], fo, fn);
#pragma unroll
                    for (int t = 0; t < VEC; ++t) S[c][t] = fmaf(S[c][t], fo, (kept ? st.v[c][t] : 0.f) * fn);
                    Se[c] = fmaf(Se[c], fo, (kept ? st.e[c] : 0.f) * fn);
                    M[c] = up ? s : M[c];
                }
            });
        if (it.slot >= 0) {  // a chunk of a long row: the raw state, folded by dot_attn_edge_combine_kernel
            float* wS = a.ws + (int64_t)it.slot * a.HD;
            float* wM = a.ws + a.n_slots * a.HD + (int64_t)it.slot * a.H;
            float* wE = a.ws + a.n_slots * (a.HD + 2 * a.H) + (int64_t)it.slot * a.HK;
#pragma unroll
            for (int c = 0; c < NCHUNK; ++c) {
                if (ht.act[c]) vstore<VEC>(wS + ht.off[c], S[c]);
                if (ht.first[c]) {
                    wM[ht.hid[c]] = M[c];
                    wM[a.n_slots * a.H + ht.hid[c]] = Z[c];
                }
                if (ej[c] >= 0) wE[ht.hid[c] * a.K + ej[c]] = Se[c];
            }
            continue;
        }
        const bool some = it.beg < it.end;  // an empty row: zeros
#pragma unroll
        for (int c = 0; c < NCHUNK; ++c) {
            if (ht.act[c]) {
                float o[VEC];
#pragma unroll
                for (int t = 0; t < VEC; ++t) o[t] = some ? a.c * (S[c][t] / Z[c]) : 0.f;
                vstore<VEC>(a.out + (int64_t)it.row * a.ldo + ht.off[c], o);
            }
            if (ht.first[c]) a.lse[(int64_t)it.row * a.ldl + ht.hid[c]] = some ? M[c] + logf(Z[c]) : 0.f;
            if (ej[c] >= 0) a.aef[(int64_t)it.row * a.ldae + ht.hid[c] * a.K + ej[c]] = some ? a.c * (Se[c] / Z[c]) : 0.f;
        }
    }
}

// One thread per (long row, column of out or of aef): the chunks' states are folded in slot order (= position order) with the sweep's
// merge, then the row's epilogue.  (A long row has at least two chunks and no chunk is empty.)
__global__ __launch_bounds__(kBlock) void dot_attn_edge_combine_kernel(DotEdgeFwdArgs a, const int32_t* long_rows, const int32_t* long_ptr,
                                                                       int64_t n_long) {
    const int W = a.HD + a.HK;
    const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gid >= n_long * W) return;
    const int64_t i = gid / W;
    const int col = (int)(gid - i * W);
    const bool edge = col >= a.HD;
    const int ce = col - a.HD;
    const int h = edge ? ce / a.K : col / a.D;
    const int row = long_rows[i], p1 = long_ptr[i + 1];
    int s = long_ptr[i];
    const float* wS = edge ? a.ws + a.n_slots * (a.HD + 2 * a.H) + ce : a.ws + col;
    const int64_t ldS = edge ? a.HK : a.HD;
    const float* wM = a.ws + a.n_slots * a.HD + h;
    const float* wZ = wM + a.n_slots * a.H;
    float M = 0.f, Z = 0.f, S = 0.f, Q = 0.f;
    const bool some = s < p1;
    if (some) {
        M = wM[(int64_t)s * a.H], Z = wZ[(int64_t)s * a.H], S = wS[(int64_t)s * ldS];
        ++s;
    }
    for (; s < p1; ++s) smx_merge<false>(M, Z, S, Q, wM[(int64_t)s * a.H], wZ[(int64_t)s * a.H], wS[(int64_t)s * ldS], 0.f);
    const float r = some ? a.c * (S / Z) : 0.f;
    if (edge) {
        a.aef[(int64_t)row * a.ldae + ce] = r;
        return;
    }
    a.out[(int64_t)row * a.ldo + col] = r;
    if (col == h * a.D) a.lse[(int64_t)row * a.ldl + h] = some ? M + logf(Z) : 0.f;
}

template <int VEC, int LANES, int NCHUNK>
__global__ __launch_bounds__(kBlock) void dot_attn_edge_bwd_dst_kernel(DotEdgeDstArgs a) {
    using Stage = DotEdgeStage<VEC, NCHUNK>;
    constexpr int U = dot_edge_unroll<VEC, NCHUNK>();
    const int lane = threadIdx.x % LANES;
    const int64_t item = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / LANES;
    if (item >= a.n_items) return;  // whole groups leave together
    const RowItem it = load_item<LANES>(a.items, item);
    const int tcols = a.hpt * a.D;
    for (int col0 = 0; col0 < a.HD; col0 += tcols) {
        const HeadTile<VEC, LANES, NCHUNK> ht(col0, min(a.HD, col0 + tcols), lane, a.D);
        float qv[NCHUNK][VEC], dv[NCHUNK][VEC], acc[NCHUNK][VEC] = {}, delta[1][NCHUNK], lse[NCHUNK];
        float qe[NCHUNK], de[NCHUNK], acce[NCHUNK] = {};
        int ej[NCHUNK];
        dot_edge_owner(ht, a.D, a.K, ej);
#pragma unroll
        for (int c = 0; c < NCHUNK; ++c) {
            float ov[VEC];
            vload<VEC>(qv[c], a.q + (int64_t)it.row * a.ldq + ht.off[c]);
            vload<VEC>(dv[c], a.dout + (int64_t)it.row * a.ldd + ht.off[c]);
            vload<VEC>(ov, a.out + (int64_t)it.row * a.ldo + ht.off[c]);
            lse[c] = a.lse[(int64_t)it.row * a.ldl + ht.head(c)];
            const int eo = ht.hid[c] * a.K + ej[c];
            qe[c] = ej[c] >= 0 ? a.qe[(int64_t)it.row * a.ldqe + eo] : 0.f;
            de[c] = ej[c] >= 0 ? a.daef[(int64_t)it.row * a.lddae + eo] : 0.f;
            const float ae = ej[c] >= 0 ? a.aef[(int64_t)it.row * a.ldae + eo] : 0.f;
            delta[0][c] = dv[c][0] * ov[0];
#pragma unroll
            for (int t = 1; t < VEC; ++t) delta[0][c] += dv[c][t] * ov[t];
            const float xd = de[c] * ae;  // (a zero product is not added: with ef = 0 delta and dd keep the plain sweep's bytes, the sign of a zero too)
            delta[0][c] = ej[c] >= 0 && xd != 0.f ? delta[0][c] + xd : delta[0][c];
        }
        ht.template total<1>(delta);
        walk_row_at<LANES, Stage, U>(
            it.beg, it.end, lane, [&](int k, bool in) { return Edge{in ? a.indices[k] : 0, in && a.keep ? a.keep[k] : -1}; },
            [&](int s, int, Stage& st, int k) {
                const float* pk = a.k + (int64_t)s * a.ldk;
                const float* pv = a.v + (int64_t)s * a.ldv;
                const float* pe = a.ef + (int64_t)k * a.ldef;
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c) {
                    vload<VEC>(st.k[c], pk + ht.off[c]);
                    vload<VEC>(st.v[c], pv + ht.off[c]);
                    st.e[c] = ej[c] >= 0 ? pe[ej[c]] : 0.f;
                }
            },
            [&](int, int w, const Stage& st, int k) {
                float p[2][NCHUNK];  // the logit's and dd's partial sums: both through the same shuffle steps
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c) {
                    p[0][c] = qv[c][0] * st.k[c][0];
                    p[1][c] = dv[c][0] * st.v[c][0];
#pragma unroll
                    for (int t = 1; t < VEC; ++t) {
                        p[0][c] += qv[c][t] * st.k[c][t];
                        p[1][c] += dv[c][t] * st.v[c][t];
                    }
                    p[0][c] = ej[c] >= 0 ? p[0][c] + qe[c] * st.e[c] : p[0][c];  // the forward's logit, product for product
                    const float xe = de[c] * st.e[c];
                    p[1][c] = ej[c] >= 0 && xe != 0.f ? p[1][c] + xe : p[1][c];
                }
                ht.template total<2>(p);
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c) {
                    const float w_a = smx_exp(a.scale * p[0][c] - lse[c]);
                    const float ck = dot_kept(w, ht.hid[c]) ? a.c : 0.f;
                    const float g = w_a * (ck * p[1][c] - delta[0][c]);
#pragma unroll
                    for (int t = 0; t < VEC; ++t) acc[c][t] = fmaf(g, st.k[c][t], acc[c][t]);
                    acce[c] = fmaf(g, st.e[c], acce[c]);
                    if (ht.first[c]) {
                        a.pw[(int64_t)k * a.H + ht.hid[c]] = ck * w_a;
                        a.ds[(int64_t)k * a.H + ht.hid[c]] = g;
                    }
                }
            });
        if (a.dq) {
            float* po = sum_row(it, a.dq, a.lddq, a.partial, a.HD);
#pragma unroll
            for (int c = 0; c < NCHUNK; ++c)
                if (ht.act[c]) {
#pragma unroll
                    for (int t = 0; t < VEC; ++t) acc[c][t] = a.scale * acc[c][t];
                    vstore<VEC>(po + ht.off[c], acc[c]);
                }
        }
        if (a.dqe) {
            float* po = sum_row(it, a.dqe, a.lddqe, a.partial + a.n_slots * a.HD, a.HK);
#pragma unroll
            for (int c = 0; c < NCHUNK; ++c)
                if (ej[c] >= 0) po[ht.hid[c] * a.K + ej[c]] = a.scale * acce[c];
        }
    }
}

struct DotEdgeFwdKern {
    template <int VEC, int LANES, int NCHUNK>
    static void launch(const DotEdgeFwdArgs& b, unsigned blocks, hipStream_t st) {
        set_kernel("bot::dot_attn_edge_kernel<%d,%d,%d>", VEC, LANES, NCHUNK);
        hipLaunchKernelGGL((dot_attn_edge_kernel<VEC, LANES, NCHUNK>), dim3(blocks), dim3(kBlock), 0, st, b);
    }
};
struct DotEdgeDstKern {
    template <int VEC, int LANES, int NCHUNK>
    static void launch(const DotEdgeDstArgs& b, unsigned blocks, hipStream_t st) {
        set_kernel("bot::dot_attn_edge_bwd_dst_kernel<%d,%d,%d>", VEC, LANES, NCHUNK);
        hipLaunchKernelGGL((dot_attn_edge_bwd_dst_kernel<VEC, LANES, NCHUNK>), dim3(blocks), dim3(kBlock), 0, st, b);
    }
};

// The widest vector of pick_vec's choice that leaves every edge column an owner: D / vec >= K (D >= K: checked by the callers)
static int dot_edge_vec(int vec, int32_t D, int32_t K) {
    while (vec > 1 && D / vec < K) vec /= 2;
    return vec;
}

}  // namespace bot

extern "C" {

#define DOT_EDGE_COMMON(name)                                                                                                              \
    BOT_REQUIRE(H >= 1 && D >= 1 && (int64_t)H * D < (1 << 24), BOT_E_RANGE, name ": H=%d D=%d (>= 1, H*D < 2^24)", H, D);              \
    BOT_REQUIRE(scale == scale, BOT_E_RANGE, name ": scale is NaN");                                                                      \
    BOT_REQUIRE(K >= 1 && K <= kDotEdgeMaxK, BOT_E_RANGE, name ": K=%d (1 <= K <= %d)", K, kDotEdgeMaxK);                               \
    BOT_REQUIRE(D >= K, BOT_E_RANGE, name ": a head of D=%d columns has no slot for each of K=%d edge columns (D >= K)", D, K);          \
    BOT_REQUIRE(p >= 0.f && p < 1.f, BOT_E_RANGE, name ": p=%g (0 <= p < 1)", (double)p);                                               \
    BOT_REQUIRE(!keep || H <= 32, BOT_E_RANGE, name ": a keep mask holds one bit per head, H=%d (<= 32)", H);

int bot_dot_attn_edge_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                          const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots, const float* q, int64_t ldq,
                          const float* k, int64_t ldk, const float* v, int64_t ldv, const float* qe, int64_t ldqe, const float* ef, int64_t ldef,
                          int32_t H, int32_t D, int32_t K, float scale, const int32_t* keep, float p, float* out, int64_t ldo, float* lse,
                          int64_t ldl, float* aef, int64_t ldae, void* workspace, bot_stream_t stream) {
    using namespace bot;
    (void)indptr;
    if (int rc = check_plan_sizes("dot_attn_edge", n_rows, nnz, n_items, n_long, n_slots)) return rc;
    DOT_EDGE_COMMON("dot_attn_edge")
    if (n_rows == 0) return 0;
    if (int rc = check_plan("dot_attn_edge", items, "items/q/qe/out/lse/aef", q && qe && out && lse && aef, nnz, "indices/k/v/ef",
                            indices && k && v && ef, n_long, "long_rows/long_ptr/workspace", long_rows && long_ptr && workspace))
        return rc;
    BOT_REQUIRE(n_long == 0 || n_slots > 0, BOT_E_RANGE, "dot_attn_edge: long rows without slots");
    const int32_t HD = H * D, HK = H * K;
    for (const float* o : {(const float*)out, (const float*)lse, (const float*)aef})
        BOT_REQUIRE(o != q && o != k && o != v && o != qe && o != ef, BOT_E_RANGE, "dot_attn_edge: an output aliases an input");
    BOT_REQUIRE(out != lse && out != aef && lse != aef, BOT_E_RANGE, "dot_attn_edge: out, lse and aef alias each other");
    BOT_REQUIRE(ldq >= HD && ldk >= HD && ldv >= HD && ldo >= HD && ldl >= H && ldqe >= HK && ldae >= HK && ldef >= K, BOT_E_RANGE,
                "dot_attn_edge: row strides smaller than the rows (ldq=%lld ldk=%lld ldv=%lld ldo=%lld H*D=%d ldl=%lld H=%d ldqe=%lld ldae=%lld "
                "H*K=%d ldef=%lld K=%d)",
                (long long)ldq, (long long)ldk, (long long)ldv, (long long)ldo, HD, (long long)ldl, H, (long long)ldqe, (long long)ldae, HK,
                (long long)ldef, K);
    BOT_REQUIRE(aligned(q, 4) && aligned(k, 4) && aligned(v, 4) && aligned(qe, 4) && aligned(ef, 4) && aligned(out, 4) && aligned(lse, 4) &&
                    aligned(aef, 4) && aligned(keep, 4) && aligned(items, 16) && aligned(workspace, 16),
                BOT_E_ALIGN, "dot_attn_edge: misaligned pointer");
    const int vec = dot_edge_vec(pick_vec(D, {ldq, ldk, ldv, ldo}, {q, k, v, out}), D, K);
    BOT_REQUIRE(dot_head_fits(D, vec), BOT_E_RANGE, "dot_attn_edge: a head of D=%d columns read %d at a time does not fit one tile of %d lanes",
                D, vec, kWave * kDotMaxChunk);
    hipStream_t st = (hipStream_t)stream;
    DotEdgeFwdArgs a{};
    a.indices = indices, a.keep = keep, a.items = reinterpret_cast<const int4*>(items), a.n_items = n_items;
    a.q = q, a.ldq = ldq, a.k = k, a.ldk = ldk, a.v = v, a.ldv = ldv, a.H = H, a.D = D, a.HD = HD;
    a.qe = qe, a.ldqe = ldqe, a.ef = ef, a.ldef = ldef, a.K = K, a.HK = HK;
    a.scale = scale, a.c = keep ? 1.f / (1.f - p) : 1.f;
    a.out = out, a.ldo = ldo, a.lse = lse, a.ldl = ldl, a.aef = aef, a.ldae = ldae;
    a.ws = static_cast<float*>(workspace), a.n_slots = n_slots;
    // (the workspace: 16-byte base, S rows of H*D floats first - H*D % vec == 0 keeps every row aligned - then M, Z and S_ef)
    dot_dispatch<DotEdgeFwdKern>(a, vec, st);
    if (int rc = hip_status("dot_attn_edge launch")) return rc;
    if (n_long > 0) {
        hipLaunchKernelGGL(dot_attn_edge_combine_kernel, dim3((unsigned)((n_long * (HD + HK) + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, a,
                           long_rows, long_ptr, n_long);
        if (int rc = hip_status("dot_attn_edge combine launch")) return rc;
    }
    return 0;
}

int bot_dot_attn_edge_bwd_dst_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items,
                                  int64_t n_items, const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots,
                                  const float* q, int64_t ldq, const float* k, int64_t ldk, const float* v, int64_t ldv, const float* qe,
                                  int64_t ldqe, const float* ef, int64_t ldef, int32_t H, int32_t D, int32_t K, float scale, const int32_t* keep,
                                  float p, const float* dout, int64_t ldd, const float* out, int64_t ldo, const float* lse, int64_t ldl,
                                  const float* aef, int64_t ldae, const float* daef, int64_t lddae, float* pw, float* ds, float* dq, int64_t lddq,
                                  float* dqe, int64_t lddqe, float* partial, bot_stream_t stream) {
    using namespace bot;
    (void)indptr;
    if (int rc = check_plan_sizes("dot_attn_edge_bwd_dst", n_rows, nnz, n_items, n_long, n_slots)) return rc;
    DOT_EDGE_COMMON("dot_attn_edge_bwd_dst")
    if (n_rows == 0) return 0;
    if (int rc = check_plan("dot_attn_edge_bwd_dst", items, "items/q/qe/dout/out/lse/aef/daef", q && qe && dout && out && lse && aef && daef, nnz,
                            "indices/k/v/ef/p/ds", indices && k && v && ef && pw && ds, n_long && (dq || dqe), "long_rows/long_ptr/partial",
                            long_rows && long_ptr && partial))
        return rc;
    BOT_REQUIRE(n_long == 0 || n_slots > 0, BOT_E_RANGE, "dot_attn_edge_bwd_dst: long rows without slots");
    const int32_t HD = H * D, HK = H * K;
    for (const float* o : {(const float*)dq, (const float*)dqe, (const float*)pw, (const float*)ds})
        BOT_REQUIRE(!o || (o != q && o != k && o != v && o != qe && o != ef && o != dout && o != out && o != lse && o != aef && o != daef),
                    BOT_E_RANGE, "dot_attn_edge_bwd_dst: an output aliases an input");
    BOT_REQUIRE(pw != ds || nnz == 0, BOT_E_RANGE, "dot_attn_edge_bwd_dst: p and ds alias each other");
    BOT_REQUIRE(!dq || dq != dqe, BOT_E_RANGE, "dot_attn_edge_bwd_dst: dq and dqe alias each other");
    BOT_REQUIRE(ldq >= HD && ldk >= HD && ldv >= HD && ldd >= HD && ldo >= HD && ldl >= H && (!dq || lddq >= HD) && ldqe >= HK && ldae >= HK &&
                    lddae >= HK && (!dqe || lddqe >= HK) && ldef >= K,
                BOT_E_RANGE,
                "dot_attn_edge_bwd_dst: row strides smaller than the rows (ldq=%lld ldk=%lld ldv=%lld ldd=%lld ldo=%lld lddq=%lld H*D=%d ldl=%lld "
                "H=%d ldqe=%lld ldae=%lld lddae=%lld lddqe=%lld H*K=%d ldef=%lld K=%d)",
                (long long)ldq, (long long)ldk, (long long)ldv, (long long)ldd, (long long)ldo, (long long)lddq, HD, (long long)ldl, H,
                (long long)ldqe, (long long)ldae, (long long)lddae, (long long)lddqe, HK, (long long)ldef, K);
    BOT_REQUIRE(aligned(q, 4) && aligned(k, 4) && aligned(v, 4) && aligned(qe, 4) && aligned(ef, 4) && aligned(dout, 4) && aligned(out, 4) &&
                    aligned(lse, 4) && aligned(aef, 4) && aligned(daef, 4) && aligned(pw, 4) && aligned(ds, 4) && aligned(dq, 4) &&
                    aligned(dqe, 4) && aligned(keep, 4) && aligned(items, 16) && aligned(partial, 16),
                BOT_E_ALIGN, "dot_attn_edge_bwd_dst: misaligned pointer");
    const int vec = dot_edge_vec(pick_vec(D, {ldq, ldk, ldv, ldd, ldo, dq ? lddq : 0}, {q, k, v, dout, out, dq}), D, K);
    BOT_REQUIRE(dot_head_fits(D, vec), BOT_E_RANGE,
                "dot_attn_edge_bwd_dst: a head of D=%d columns read %d at a time does not fit one tile of %d lanes", D, vec, kWave * kDotMaxChunk);
    hipStream_t st = (hipStream_t)stream;
    DotEdgeDstArgs a{};
    a.indices = indices, a.keep = keep, a.items = reinterpret_cast<const int4*>(items), a.n_items = n_items;
    a.q = q, a.ldq = ldq, a.k = k, a.ldk = ldk, a.v = v, a.ldv = ldv, a.H = H, a.D = D, a.HD = HD;
    a.qe = qe, a.ldqe = ldqe, a.ef = ef, a.ldef = ldef, a.K = K, a.HK = HK;
    a.scale = scale, a.c = keep ? 1.f / (1.f - p) : 1.f;
    a.dout = dout, a.ldd = ldd, a.out = out, a.ldo = ldo, a.lse = lse, a.ldl = ldl, a.aef = aef, a.ldae = ldae, a.daef = daef, a.lddae = lddae;
    a.pw = pw, a.ds = ds, a.dq = dq, a.lddq = lddq, a.dqe = dqe, a.lddqe = lddqe, a.partial = partial, a.n_slots = n_slots;
    dot_dispatch<DotEdgeDstKern>(a, vec, st);
    if (int rc = hip_status("dot_attn_edge_bwd_dst launch")) return rc;
    if (n_long > 0) {
        if (dq) launch_sum_combine(partial, HD, dq, lddq, long_rows, long_ptr, n_long, st);
        if (dqe) launch_sum_combine(partial + n_slots * HD, HK, dqe, lddqe, long_rows, long_ptr, n_long, st);
        if (int rc = hip_status("dot_attn_edge_bwd_dst combine launch")) return rc;
    }
    return 0;
}

}  // extern "C"
