// Dot-product attention over a node's in-edges (include/bot_gnn.h "Dot-product attention", "Dot-product attention with edge features")
// for gfx950: the layer of UniMP (Shi et al., "Masked Label Prediction", IJCAI 2021, arXiv:2009.03509), PyG's TransformerConv and DGL's
// DotGatConv (bot_amd.nn, `ops.dot_attention`), and PyG's TransformerConv(edge_dim=K) (EdgeTransformerConv, `ops.dot_attention_edge`).
// Per head h, with s_k = scale * sum_d q[v,h,d] k[u_k,h,d] over the in-edges k of v, keep_k,h in {0, 1} the attention-dropout mask and
// c = 1 / (1 - p):
//   forward        lse[v,h] = log sum_k exp(s_k),  a_k = exp(s_k - lse[v,h]),  out[v,h,:] = c sum_k keep_k a_k v[u_k,h,:]   (rows = destinations: CSC)
//                  an empty row gives out = 0, lse = 0
//   backward, dst  delta[v,h] = sum_d dout[v,h,d] out[v,h,d],  dd_k = sum_d dout[v,h,d] v[u_k,h,d],  p_k = c keep_k a_k,
//                  ds_k = a_k (c keep_k dd_k - delta[v,h]),  dq[v,h,:] = scale sum_k ds_k k[u_k,h,:];  stores p[k,h], ds[k,h]          (the CSC)
//   backward, src  dk[u,h,:] = scale sum_j ds[pos_j,h] q[v_j,h,:],  dv[u,h,:] = sum_j p[pos_j,h] dout[v_j,h,:]             (rows = sources: CSR)
//
// The EDGE instances add K raw edge features to the key and the value.  With E_e = W ef_e the edge encoder's row of the in-edge e = u -> v
// and W viewed as [H, D, K], PyG's layer is s_e = scale <q[v,h], k[u,h] + E_e[h]>, out[v,h] = sum_e p_e (v[u,h] + E_e[h]).  Everything
// the edge term touches is linear, so the encoder stays OUTSIDE the sweep:
//   <q[v,h], E_e[h]> = <qe[v,h], ef_e>       qe[v,h,:]  = q[v,h,:] W[h]      a dense product before the sweep
//   sum_e p_e E_e[h] = W[h] aef[v,h,:]       aef[v,h,:] = sum_e p_e ef_e     reduced here, projected after the sweep
// The sweeps carry K raw floats per edge and K accumulators per head; the weights never enter a kernel.
//   forward        s_k = scale (<q[v,h], k[u_k,h]> + <qe[v,h], ef_k>),  lse, a_k, out as above,  aef[v,h,:] = c sum_k keep_k a_k ef_k
//   backward, dst  delta[v,h] = <dout[v,h], out[v,h]> + <daef[v,h], aef[v,h]>,  dd_k = <dout[v,h], v[u_k,h]> + <daef[v,h], ef_k>,
//                  p_k, ds_k, dq as above,  dqe[v,h,:] = scale sum_k ds_k ef_k
// dk and dv depend on the edge term only through the stored p and ds: one backward over the sources serves both.
//
// All three are the lane-group row sweep that sweep.h describes (load_item, ColTile's layout, walk_row) over the H*D columns; VEC divides
// D, so a lane's vector never straddles two heads.  Heads are independent, so a row wider than one tile (64 lanes x VEC x NCHUNK, NCHUNK
// up to 6: 3 x 250 with 8-byte lanes is one tile) walks tiles made of WHOLE heads; the ids are read again per tile.  One head must fit a
// tile: D <= 64 VEC 6, else BOT_E_RANGE (the caller runs the tensor form).
//
// Forward: ONE launch forms logits, online softmax and aggregation from one gather; nothing is stored per edge and [E, H, D] never
// exists.  The row owner keeps q[v] in registers; per neighbour two row gathers, k[u] and v[u] - one when they are the same rows (the
// SHARED instances: DotGatConv).  The per-lane partial dot product is reduced over the head's lanes and handed to every lane of the
// head (HeadTile::total): in one-chunk instances a segmented scan over the head's lanes (only the steps shorter than a head run) and
// one cross-lane read from the head's last lane; in the wide instances, whose few heads span 64-lane chunks, one masked 64-lane
// butterfly per head of the tile.  The order of the sum over d is fixed per instance.  Each lane then keeps (M, Z) once per chunk - the
// same value on all lanes of a head - and S per column, with ONE exponential per lane, chunk and neighbour (smx.h: the merge of
// spmm_softmax.hip with Z2 = 1).  The first neighbour initialises the state; Z counts every edge, S only the kept ones.  Epilogue: out
// = c * (S / Z) by a true division (uniform weights: float32(sum) / float32(deg) bit for bit), lse = M + log Z.  The chunks of a long
// row leave S per column and raw (M, Z) per head in the workspace; dot_attn_combine_kernel folds them in slot order with the same
// merge and applies the same epilogue.  keep: one int32 per position, bit h = head h is kept, read beside the ids (Edge.word).
//
// Backward over destinations: the same gather; the row owner holds q[v], dout[v], lse[v,.] and delta[v,.] (formed once per row from
// out[v]); per neighbour the two head reductions s and dd go through the same shuffle steps.  dq is a row-owner sum in registers, long
// rows through `partial` and launch_sum_combine.  Backward over sources: per out-edge the destination's q and dout rows and the 2 H
// words p, ds through pos; no reduction, no exponential.  No float atomics anywhere: all three repeat their bytes.
//
// The edge term is laid over the same lanes, behind `if constexpr (EDGE)` (the EDGE instances are non-shared): the j-th vector slot of
// a head, (column - h D) / VEC == j < K, OWNS edge column j - one qe word, one staged ef word per neighbour in flight and one
// accumulator.  The ef row of a position is one coalesced read of K words by the owning lanes of every head; ef is in POSITION order, so
// the fetch reads it at the position the walk hands it, and the edge word stays the keep mask.  The owner's product qe ef joins the lane's
// partial logit BEFORE the head reduction, so the order of the sum is fixed per instance and there is still one exponential per lane,
// chunk and neighbour.  Every column needs an owner: D / VEC >= K, and the entry points narrow VEC until that holds.  With ef = 0 every
// output keeps the plain instance's bytes.
//
// HBM model (4-byte words; HD = H*D, HK = H*K): forward 4 [E (1 + 2 HD) + n_dst (2 HD + H)] (ids, a k and a v row per edge; q read, out
// and lse written per row), E (1 + HD) when k and v are shared; backward over destinations 4 [E (1 + 2 HD + 2 H) + n_dst (4 HD + 2 H)]
// (ids, k and v rows, p and ds written per edge; q, dout, out read, dq written, lse read per row; the keep word adds E); backward over
// sources 4 [E (2 + 2 HD + 2 H) + 3 n_src HD] (ids and positions, q and dout rows, p and ds per edge; dk and dv written per row).
// With edge features: forward 4 [E (1 + 2 HD + K) + n_dst (2 HD + H + 2 HK)]; backward over destinations 4 [E (1 + 2 HD + K + 2 H) +
// n_dst (4 HD + 2 H + 4 HK)] (the keep word adds E to each).
#include "dot.h"

#include <cmath>
#include <cstdio>
#include <initializer_list>

namespace bot {

constexpr int kDotEdgeMaxK = 16;  // the widest raw edge feature (include/bot_gnn.h)

// The arguments of the two sweeps over destinations.  The fields from qe on belong to the EDGE instances: the plain entry points
// leave them 0 and the plain instances never read them.
struct DotFwdArgs : DotPlan {
    const int32_t* keep;  // NULL: every edge kept
    float c;
    const float* q;
    int64_t ldq;
    const float* k;
    int64_t ldk;
    const float* v;
    int64_t ldv;
    float* out;
    int64_t ldo;
    float* lse;
    int64_t ldl;
    float* ws;  // S [n_slots, HD], M [n_slots, H], Z [n_slots, H], S_ef [n_slots, HK]: the chunks' states of the long rows
    int64_t n_slots;
    const float* qe;  // [n_dst, H K]
    int64_t ldqe;
    const float* ef;  // [E, K], position order
    int64_t ldef;
    int32_t K, HK;
    float* aef;  // [n_dst, H K]
    int64_t ldae;
};

struct DotDstArgs : DotPlan {
    const int32_t* keep;
    float c;
    const float* q;
    int64_t ldq;
    const float* k;
    int64_t ldk;
    const float* v;
    int64_t ldv;
    const float* dout;
    int64_t ldd;
    const float* out;
    int64_t ldo;
    const float* lse;
    int64_t ldl;
    float* pw;  // [E, H] p and ds, written
    float* ds;
    float* dq;  // NULL: not asked for
    int64_t lddq;
    float* partial;  // dq [n_slots, HD], then dqe [n_slots, HK]: chunk sums of the long rows
    const float* qe;
    int64_t ldqe;
    const float* ef;
    int64_t ldef;
    int32_t K, HK;
    const float* aef;
    int64_t ldae;
    const float* daef;
    int64_t lddae;
    float* dqe;  // NULL: not asked for
    int64_t lddqe;
    int64_t n_slots;
};

struct DotSrcArgs : DotPlan {
    const int32_t* pos;
    const float* q;
    int64_t ldq;
    const float* dout;
    int64_t ldd;
    const float* pw;  // [E, H] p and ds, read through pos
    const float* ds;
    float* dk;  // NULL: not asked for; dk == dv: one output that holds dk + dv
    int64_t lddk;
    float* dv;
    int64_t lddv;
    float* partial;  // [2][n_slots, HD] chunk sums of the long rows: dk's plane, then dv's
    int64_t n_slots;
};

template <bool SHARED, bool EDGE, int VEC, int NCHUNK>
struct DotStage {
    static_assert(!(SHARED && EDGE), "the edge sweeps gather k and v separately");
    float k[NCHUNK][VEC];
    float v[SHARED ? 1 : NCHUNK][SHARED ? 1 : VEC];
    float e[EDGE ? NCHUNK : 1];  // EDGE: the owner's word of the position's ef row, 0 elsewhere
    __device__ __forceinline__ float val(int c, int t) const {
        if constexpr (SHARED) return k[c][t];
        else return v[c][t];
    }
};

// The edge column each of a lane's slots owns, or -1
template <int VEC, int LANES, int NCHUNK>
__device__ __forceinline__ void dot_edge_owner(const HeadTile<VEC, LANES, NCHUNK>& ht, int D, int K, int (&ej)[NCHUNK]) {
#pragma unroll
    for (int c = 0; c < NCHUNK; ++c) {
        const int j = (ht.off[c] - ht.head(c) * D) / VEC;
        ej[c] = ht.act[c] && j < K ? j : -1;
    }
}

// A neighbour's rows into the staging slot: k[u], v[u] unless they are the same rows, and the owned word of the position's ef row
template <bool SHARED, bool EDGE, int VEC, int LANES, int NCHUNK, class Args>
__device__ __forceinline__ void dot_fetch(const Args& a, const HeadTile<VEC, LANES, NCHUNK>& ht, const int (&ej)[NCHUNK], int s, int k,
                                          DotStage<SHARED, EDGE, VEC, NCHUNK>& st) {
    const float* pk = a.k + (int64_t)s * a.ldk;
    const float* pv = a.v + (int64_t)s * a.ldv;
    const float* pe = EDGE ? a.ef + (int64_t)k * a.ldef : nullptr;
#pragma unroll
    for (int c = 0; c < NCHUNK; ++c) {
        vload<VEC>(st.k[c], pk + ht.off[c]);
        if constexpr (!SHARED) vload<VEC>(st.v[c], pv + ht.off[c]);
        if constexpr (EDGE) st.e[c] = ej[c] >= 0 ? pe[ej[c]] : 0.f;
    }
}

template <bool SHARED, bool EDGE, int VEC, int LANES, int NCHUNK>
__global__ __launch_bounds__(kBlock) void dot_attn_kernel(DotFwdArgs a) {
    using Stage = DotStage<SHARED, EDGE, VEC, NCHUNK>;
    constexpr int U = dot_unroll(NCHUNK * VEC * (SHARED ? 1 : 2));  // (the staged ef word is one register per chunk beside 2 VEC)
    const int lane = threadIdx.x % LANES;
    const int64_t item = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / LANES;
    if (item >= a.n_items) return;  // whole groups leave together
    const RowItem it = load_item<LANES>(a.items, item);
    const int tcols = a.hpt * a.D;
    for (int col0 = 0; col0 < a.HD; col0 += tcols) {  // groups narrower than a wavefront have one tile (DotLaunch)
        const HeadTile<VEC, LANES, NCHUNK> ht(col0, min(a.HD, col0 + tcols), lane, a.D);
        float qv[NCHUNK][VEC], M[NCHUNK] = {}, Z[NCHUNK] = {}, S[NCHUNK][VEC] = {};
        [[maybe_unused]] float qe[NCHUNK], Se[NCHUNK] = {};
        int ej[NCHUNK];
        if constexpr (EDGE) dot_edge_owner(ht, a.D, a.K, ej);
#pragma unroll
        for (int c = 0; c < NCHUNK; ++c) {
            vload<VEC>(qv[c], a.q + (int64_t)it.row * a.ldq + ht.off[c]);
            if constexpr (EDGE) qe[c] = ej[c] >= 0 ? a.qe[(int64_t)it.row * a.ldqe + ht.hid[c] * a.K + ej[c]] : 0.f;
        }
        walk_row<LANES, Stage, U>(
            it.beg, it.end, lane, [&](int k, bool in) { return Edge{in ? a.indices[k] : 0, in && a.keep ? a.keep[k] : -1}; },
            [&](int s, int, Stage& st, int k) { dot_fetch(a, ht, ej, s, k, st); },
            [&](int, int w, const Stage& st, int k) {
                float p[1][NCHUNK];
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c) {
                    p[0][c] = qv[c][0] * st.k[c][0];
#pragma unroll
                    for (int t = 1; t < VEC; ++t) p[0][c] += qv[c][t] * st.k[c][t];
                    if constexpr (EDGE) p[0][c] = ej[c] >= 0 ? p[0][c] + qe[c] * st.e[c] : p[0][c];  // the edge term: before the head reduction
                }
                ht.template total<1>(p);
                if (k == it.beg) {  // the first neighbour is the state
#pragma unroll
                    for (int c = 0; c < NCHUNK; ++c) {
                        const bool kept = dot_kept(w, ht.hid[c]);
                        M[c] = a.scale * p[0][c];
                        Z[c] = 1.f;
#pragma unroll
                        for (int t = 0; t < VEC; ++t) S[c][t] = kept ? st.val(c, t) : 0.f;
                        if constexpr (EDGE) Se[c] = kept ? st.e[c] : 0.f;
                    }
                    return;
                }
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c) {  // smx_merge with (M2, Z2, S2) = (s, 1, kept ? v : 0): one exponential per lane and chunk
                    const bool kept = dot_kept(w, ht.hid[c]);
                    const float s = a.scale * p[0][c];
                    const float d = s - M[c];
                    const float e = smx_exp(-fabsf(d));
                    const bool up = d > 0.f;
                    const float fo = up ? e : 1.f, fn = up ? 1.f : e;
                    Z[c] = fmaf(Z[c], fo, fn);
#pragma unroll
                    for (int t = 0; t < VEC; ++t) S[c][t] = fmaf(S[c][t], fo, (kept ? st.val(c, t) : 0.f) * fn);
                    if constexpr (EDGE) Se[c] = fmaf(Se[c], fo, (kept ? st.e[c] : 0.f) * fn);
                    M[c] = up ? s : M[c];
                }
            });
        if (it.slot >= 0) {  // a chunk of a long row: the raw state, folded by dot_attn_combine_kernel
            float* wS = a.ws + (int64_t)it.slot * a.HD;
            float* wM = a.ws + a.n_slots * a.HD + (int64_t)it.slot * a.H;
            float* wE = EDGE ? a.ws + a.n_slots * (a.HD + 2 * a.H) + (int64_t)it.slot * a.HK : nullptr;
#pragma unroll
            for (int c = 0; c < NCHUNK; ++c) {
                if (ht.act[c]) vstore<VEC>(wS + ht.off[c], S[c]);
                if (ht.first[c]) {
                    wM[ht.hid[c]] = M[c];
                    wM[a.n_slots * a.H + ht.hid[c]] = Z[c];
                }
                if constexpr (EDGE)
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
            if constexpr (EDGE)
                if (ej[c] >= 0) a.aef[(int64_t)it.row * a.ldae + ht.hid[c] * a.K + ej[c]] = some ? a.c * (Se[c] / Z[c]) : 0.f;
        }
    }
}

// One thread per (long row, column of out or - EDGE - of aef): the chunks' states are folded in slot order (= position order) with the
// sweep's merge, then the row's epilogue.  (A long row has at least two chunks and no chunk is empty.)
template <bool EDGE>
__global__ __launch_bounds__(kBlock) void dot_attn_combine_kernel(DotFwdArgs a, const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long) {
    int W = a.HD;
    if constexpr (EDGE) W += a.HK;
    const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gid >= n_long * W) return;
    const int64_t i = gid / W;
    const int col = (int)(gid - i * W);
    int h = col / a.D;
    const float* wS = a.ws + col;
    int64_t ldS = a.HD;
    bool edge = false;
    if constexpr (EDGE) {
        edge = col >= a.HD;
        if (edge) h = (col - a.HD) / a.K, wS = a.ws + a.n_slots * (a.HD + 2 * a.H) + (col - a.HD), ldS = a.HK;
    }
    const int row = long_rows[i], p1 = long_ptr[i + 1];
    int s = long_ptr[i];
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
        a.aef[(int64_t)row * a.ldae + (col - a.HD)] = r;
        return;
    }
    a.out[(int64_t)row * a.ldo + col] = r;
    if (col == h * a.D) a.lse[(int64_t)row * a.ldl + h] = some ? M + logf(Z) : 0.f;
}

template <bool SHARED, bool EDGE, int VEC, int LANES, int NCHUNK>
__global__ __launch_bounds__(kBlock) void dot_attn_bwd_dst_kernel(DotDstArgs a) {
    using Stage = DotStage<SHARED, EDGE, VEC, NCHUNK>;
    constexpr int U = dot_unroll(NCHUNK * VEC * (SHARED ? 1 : 2));
    const int lane = threadIdx.x % LANES;
    const int64_t item = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / LANES;
    if (item >= a.n_items) return;  // whole groups leave together
    const RowItem it = load_item<LANES>(a.items, item);
    const int tcols = a.hpt * a.D;
    for (int col0 = 0; col0 < a.HD; col0 += tcols) {
        const HeadTile<VEC, LANES, NCHUNK> ht(col0, min(a.HD, col0 + tcols), lane, a.D);
        float qv[NCHUNK][VEC], dv[NCHUNK][VEC], acc[NCHUNK][VEC] = {}, delta[1][NCHUNK], lse[NCHUNK];
        [[maybe_unused]] float qe[NCHUNK], de[NCHUNK], acce[NCHUNK] = {};
        int ej[NCHUNK];
        if constexpr (EDGE) dot_edge_owner(ht, a.D, a.K, ej);
#pragma unroll
        for (int c = 0; c < NCHUNK; ++c) {
            float ov[VEC];
            vload<VEC>(qv[c], a.q + (int64_t)it.row * a.ldq + ht.off[c]);
            vload<VEC>(dv[c], a.dout + (int64_t)it.row * a.ldd + ht.off[c]);
            vload<VEC>(ov, a.out + (int64_t)it.row * a.ldo + ht.off[c]);
            lse[c] = a.lse[(int64_t)it.row * a.ldl + ht.head(c)];
            delta[0][c] = dv[c][0] * ov[0];
#pragma unroll
            for (int t = 1; t < VEC; ++t) delta[0][c] += dv[c][t] * ov[t];
            if constexpr (EDGE) {
                const int eo = ht.hid[c] * a.K + ej[c];
                qe[c] = ej[c] >= 0 ? a.qe[(int64_t)it.row * a.ldqe + eo] : 0.f;
                de[c] = ej[c] >= 0 ? a.daef[(int64_t)it.row * a.lddae + eo] : 0.f;
                const float ae = ej[c] >= 0 ? a.aef[(int64_t)it.row * a.ldae + eo] : 0.f;
                const float xd = de[c] * ae;  // (a zero product is not added: with ef = 0 delta and dd keep the plain sweep's bytes, the sign of a zero too)
                delta[0][c] = ej[c] >= 0 && xd != 0.f ? delta[0][c] + xd : delta[0][c];
            }
        }
        ht.template total<1>(delta);
        walk_row<LANES, Stage, U>(
            it.beg, it.end, lane, [&](int k, bool in) { return Edge{in ? a.indices[k] : 0, in && a.keep ? a.keep[k] : -1}; },
            [&](int s, int, Stage& st, int k) { dot_fetch(a, ht, ej, s, k, st); },
            [&](int, int w, const Stage& st, int k) {
                float p[2][NCHUNK];  // the logit's and dd's partial sums: both through the same shuffle steps
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c) {
                    p[0][c] = qv[c][0] * st.k[c][0];
                    p[1][c] = dv[c][0] * st.val(c, 0);
#pragma unroll
                    for (int t = 1; t < VEC; ++t) {
                        p[0][c] += qv[c][t] * st.k[c][t];
                        p[1][c] += dv[c][t] * st.val(c, t);
                    }
                    if constexpr (EDGE) {
                        p[0][c] = ej[c] >= 0 ? p[0][c] + qe[c] * st.e[c] : p[0][c];  // the forward's logit, product for product
                        const float xe = de[c] * st.e[c];
                        p[1][c] = ej[c] >= 0 && xe != 0.f ? p[1][c] + xe : p[1][c];
                    }
                }
                ht.template total<2>(p);
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c) {
                    const float w_a = smx_exp(a.scale * p[0][c] - lse[c]);
                    const float ck = dot_kept(w, ht.hid[c]) ? a.c : 0.f;
                    const float g = w_a * (ck * p[1][c] - delta[0][c]);
#pragma unroll
                    for (int t = 0; t < VEC; ++t) acc[c][t] = fmaf(g, st.k[c][t], acc[c][t]);
                    if constexpr (EDGE) acce[c] = fmaf(g, st.e[c], acce[c]);
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
        if constexpr (EDGE)
            if (a.dqe) {
                float* po = sum_row(it, a.dqe, a.lddqe, a.partial + a.n_slots * a.HD, a.HK);
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c)
                    if (ej[c] >= 0) po[ht.hid[c] * a.K + ej[c]] = a.scale * acce[c];
            }
    }
}

template <int VEC, int NCHUNK>
struct DotSrcStage {
    float q[NCHUNK][VEC], d[NCHUNK][VEC], p[NCHUNK], s[NCHUNK];
};

// rows = sources; dk and dv may each be NULL; dk == dv: one output that holds dk + dv (k and v shared)
template <int VEC, int LANES, int NCHUNK>
__global__ __launch_bounds__(kBlock) void dot_attn_bwd_src_kernel(DotSrcArgs a) {
    using Stage = DotSrcStage<VEC, NCHUNK>;
    constexpr int U = dot_unroll(NCHUNK * (2 * VEC + 2));
    const int lane = threadIdx.x % LANES;
    const int64_t item = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / LANES;
    if (item >= a.n_items) return;  // whole groups leave together
    const RowItem it = load_item<LANES>(a.items, item);
    const int tcols = a.hpt * a.D;
    const bool both = a.dk == a.dv;
    for (int col0 = 0; col0 < a.HD; col0 += tcols) {
        const HeadTile<VEC, LANES, NCHUNK> ht(col0, min(a.HD, col0 + tcols), lane, a.D);
        float ak[NCHUNK][VEC] = {}, av[NCHUNK][VEC] = {};
        walk_row<LANES, Stage, U>(
            it.beg, it.end, lane, [&](int j, bool in) { return in ? Edge{a.indices[j], a.pos[j]} : Edge{0, 0}; },
            [&](int s, int w, Stage& st, int) {
                const float* pq = a.q + (int64_t)s * a.ldq;
                const float* pd = a.dout + (int64_t)s * a.ldd;
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c) {
                    vload<VEC>(st.q[c], pq + ht.off[c]);
                    vload<VEC>(st.d[c], pd + ht.off[c]);
                    st.p[c] = a.pw[(int64_t)w * a.H + ht.head(c)];
                    st.s[c] = a.ds[(int64_t)w * a.H + ht.head(c)];
                }
            },
            [&](int, int, const Stage& st, int) {
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c)
#pragma unroll
                    for (int t = 0; t < VEC; ++t) {
                        ak[c][t] = fmaf(st.s[c], st.q[c][t], ak[c][t]);
                        av[c][t] = fmaf(st.p[c], st.d[c][t], av[c][t]);
                    }
            });
#pragma unroll
        for (int c = 0; c < NCHUNK; ++c)
#pragma unroll
            for (int t = 0; t < VEC; ++t) {
                ak[c][t] = a.scale * ak[c][t];
                if (both) ak[c][t] = ak[c][t] + av[c][t];
            }
        float* w1 = a.partial + a.n_slots * a.HD;  // the second plane of the chunk sums
#pragma unroll
        for (int c = 0; c < NCHUNK; ++c)
            if (ht.act[c]) {
                if (a.dk) vstore<VEC>(sum_row(it, a.dk, a.lddk, a.partial, a.HD) + ht.off[c], ak[c]);
                if (a.dv && !both) vstore<VEC>(sum_row(it, a.dv, a.lddv, w1, a.HD) + ht.off[c], av[c]);
            }
    }
}

// The launch shims name the instance for bot_last_kernel: the edge instances keep a name of their own, without the SHARED digit
template <bool SHARED, bool EDGE>
struct DotFwdKern {
    template <int VEC, int LANES, int NCHUNK>
    static void launch(const DotFwdArgs& b, unsigned blocks, hipStream_t st) {
        if constexpr (EDGE) set_kernel("bot::dot_attn_edge_kernel<%d,%d,%d>", VEC, LANES, NCHUNK);
        else set_kernel("bot::dot_attn_kernel<%d,%d,%d,%d>", (int)SHARED, VEC, LANES, NCHUNK);
        hipLaunchKernelGGL((dot_attn_kernel<SHARED, EDGE, VEC, LANES, NCHUNK>), dim3(blocks), dim3(kBlock), 0, st, b);
    }
};
template <bool SHARED, bool EDGE>
struct DotDstKern {
    template <int VEC, int LANES, int NCHUNK>
    static void launch(const DotDstArgs& b, unsigned blocks, hipStream_t st) {
        if constexpr (EDGE) set_kernel("bot::dot_attn_edge_bwd_dst_kernel<%d,%d,%d>", VEC, LANES, NCHUNK);
        else set_kernel("bot::dot_attn_bwd_dst_kernel<%d,%d,%d,%d>", (int)SHARED, VEC, LANES, NCHUNK);
        hipLaunchKernelGGL((dot_attn_bwd_dst_kernel<SHARED, EDGE, VEC, LANES, NCHUNK>), dim3(blocks), dim3(kBlock), 0, st, b);
    }
};
struct DotSrcKern {
    template <int VEC, int LANES, int NCHUNK>
    static void launch(const DotSrcArgs& b, unsigned blocks, hipStream_t st) {
        set_kernel("bot::dot_attn_bwd_src_kernel<%d,%d,%d>", VEC, LANES, NCHUNK);
        hipLaunchKernelGGL((dot_attn_bwd_src_kernel<VEC, LANES, NCHUNK>), dim3(blocks), dim3(kBlock), 0, st, b);
    }
};

// ---- what the entry points check, each under the entry point's name `who` ----

// H, D and scale; the edge entry points' K; the keep mask's p and heads (the sweep over the sources has neither: edge false, p 0, no keep)
static int dot_check_common(const char* who, int32_t H, int32_t D, float scale, bool edge, int32_t K, const int32_t* keep, float p) {
    BOT_REQUIRE(H >= 1 && D >= 1 && (int64_t)H * D < (1 << 24), BOT_E_RANGE, "%s: H=%d D=%d (>= 1, H*D < 2^24)", who, H, D);
    BOT_REQUIRE(scale == scale, BOT_E_RANGE, "%s: scale is NaN", who);
    if (edge) {
        BOT_REQUIRE(K >= 1 && K <= kDotEdgeMaxK, BOT_E_RANGE, "%s: K=%d (1 <= K <= %d)", who, K, kDotEdgeMaxK);
        BOT_REQUIRE(D >= K, BOT_E_RANGE, "%s: a head of D=%d columns has no slot for each of K=%d edge columns (D >= K)", who, D, K);
    }
    BOT_REQUIRE(p >= 0.f && p < 1.f, BOT_E_RANGE, "%s: p=%g (0 <= p < 1)", who, (double)p);
    BOT_REQUIRE(!keep || H <= 32, BOT_E_RANGE, "%s: a keep mask holds one bit per head, H=%d (<= 32)", who, H);
    return 0;
}

// No output (NULL: not asked for) is one of the inputs
static int dot_check_alias(const char* who, std::initializer_list<const void*> outs, std::initializer_list<const void*> ins) {
    for (const void* o : outs)
        for (const void* i : ins) BOT_REQUIRE(!o || o != i, BOT_E_RANGE, "%s: an output aliases an input", who);
    return 0;
}

struct DotRows {
    const char* ld;  // the stride's name
    int64_t stride;
    int32_t cols;
};
static int dot_check_strides(const char* who, std::initializer_list<DotRows> rows) {
    for (const DotRows& r : rows)
        BOT_REQUIRE(r.stride >= r.cols, BOT_E_RANGE, "%s: row strides smaller than the rows (%s=%lld, a row has %d columns)", who, r.ld,
                    (long long)r.stride, r.cols);
    return 0;
}

// 4-byte operands (NULL passes), and the 16-byte plan items and workspace
static int dot_check_aligned(const char* who, std::initializer_list<const void*> words, const void* items, const void* workspace) {
    bool ok = aligned(items, 16) && aligned(workspace, 16);
    for (const void* p : words) ok = ok && aligned(p, 4);
    BOT_REQUIRE(ok, BOT_E_ALIGN, "%s: misaligned pointer", who);
    return 0;
}

static int dot_check_head(const char* who, int32_t D, int vec) {
    BOT_REQUIRE(dot_head_fits(D, vec), BOT_E_RANGE, "%s: a head of D=%d columns read %d at a time does not fit one tile of %d lanes", who, D, vec,
                kWave * kDotMaxChunk);
    return 0;
}

static int dot_status(const char* who, const char* step) {
    char what[64];
    snprintf(what, sizeof what, "%s %s", who, step);
    return hip_status(what);
}

// The widest vector of pick_vec's choice that leaves every edge column an owner: D / vec >= K (D >= K: dot_check_common)
static int dot_edge_vec(int vec, int32_t D, int32_t K) {
    while (vec > 1 && D / vec < K) vec /= 2;
    return vec;
}

// bot_dot_attn_f32 / bot_dot_attn_edge_f32 on their operands in `a` (the plain entry point: no edge operands, K = 0)
template <bool EDGE>
static int dot_forward(const char* who, DotFwdArgs a, int64_t n_rows, int64_t nnz, const int32_t* long_rows, const int32_t* long_ptr,
                       int64_t n_long, float p, hipStream_t st) {
    if (int rc = check_plan_sizes(who, n_rows, nnz, a.n_items, n_long, a.n_slots)) return rc;
    if (int rc = dot_check_common(who, a.H, a.D, a.scale, EDGE, a.K, a.keep, p)) return rc;
    if (n_rows == 0) return 0;
    if (int rc = check_plan(who, a.items, EDGE ? "items/q/qe/out/lse/aef" : "items/q/out/lse", a.q && a.out && a.lse && (!EDGE || (a.qe && a.aef)),
                            nnz, EDGE ? "indices/k/v/ef" : "indices/k/v", a.indices && a.k && a.v && (!EDGE || a.ef), n_long,
                            "long_rows/long_ptr/workspace", long_rows && long_ptr && a.ws))
        return rc;
    BOT_REQUIRE(n_long == 0 || a.n_slots > 0, BOT_E_RANGE, "%s: long rows without slots", who);
    a.HD = a.H * a.D, a.HK = a.H * a.K;
    if (int rc = dot_check_alias(who, {a.out, a.lse, a.aef}, {a.q, a.k, a.v, a.qe, a.ef})) return rc;
    BOT_REQUIRE(a.out != a.lse && (!EDGE || (a.out != a.aef && a.lse != a.aef)), BOT_E_RANGE, "%s: the outputs alias each other", who);
    if (int rc = dot_check_strides(who, {{"ldq", a.ldq, a.HD}, {"ldk", a.ldk, a.HD}, {"ldv", a.ldv, a.HD}, {"ldo", a.ldo, a.HD}, {"ldl", a.ldl, a.H},
                                         {"ldqe", a.ldqe, a.HK}, {"ldae", a.ldae, a.HK}, {"ldef", a.ldef, a.K}}))
        return rc;
    if (int rc = dot_check_aligned(who, {a.q, a.k, a.v, a.qe, a.ef, a.out, a.lse, a.aef, a.keep}, a.items, a.ws)) return rc;
    int vec = pick_vec(a.D, {a.ldq, a.ldk, a.ldv, a.ldo}, {a.q, a.k, a.v, a.out});
    if (EDGE) vec = dot_edge_vec(vec, a.D, a.K);
    if (int rc = dot_check_head(who, a.D, vec)) return rc;
    a.c = a.keep ? 1.f / (1.f - p) : 1.f;
    // (the workspace: 16-byte base, S rows of H*D floats first - H*D % vec == 0 keeps every row aligned - then M, Z and S_ef)
    if constexpr (EDGE) dot_dispatch<DotFwdKern<false, true>>(a, vec, st);
    else if (a.k == a.v && a.ldk == a.ldv) dot_dispatch<DotFwdKern<true, false>>(a, vec, st);
    else dot_dispatch<DotFwdKern<false, false>>(a, vec, st);
    if (int rc = dot_status(who, "launch")) return rc;
    if (n_long > 0) {
        hipLaunchKernelGGL(dot_attn_combine_kernel<EDGE>, dim3((unsigned)((n_long * (a.HD + a.HK) + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, a,
                           long_rows, long_ptr, n_long);
        if (int rc = dot_status(who, "combine launch")) return rc;
    }
    return 0;
}

// bot_dot_attn_bwd_dst_f32 / bot_dot_attn_edge_bwd_dst_f32 likewise (the plain entry point has no n_slots either)
template <bool EDGE>
static int dot_backward_dst(const char* who, DotDstArgs a, int64_t n_rows, int64_t nnz, const int32_t* long_rows, const int32_t* long_ptr,
                            int64_t n_long, float p, hipStream_t st) {
    if (int rc = check_plan_sizes(who, n_rows, nnz, a.n_items, n_long, a.n_slots)) return rc;
    if (int rc = dot_check_common(who, a.H, a.D, a.scale, EDGE, a.K, a.keep, p)) return rc;
    if (n_rows == 0) return 0;
    if (int rc = check_plan(who, a.items, EDGE ? "items/q/qe/dout/out/lse/aef/daef" : "items/q/dout/out/lse",
                            a.q && a.dout && a.out && a.lse && (!EDGE || (a.qe && a.aef && a.daef)), nnz,
                            EDGE ? "indices/k/v/ef/p/ds" : "indices/k/v/p/ds", a.indices && a.k && a.v && a.pw && a.ds && (!EDGE || a.ef),
                            n_long && (a.dq || a.dqe), "long_rows/long_ptr/partial", long_rows && long_ptr && a.partial))
        return rc;
    BOT_REQUIRE(!EDGE || n_long == 0 || a.n_slots > 0, BOT_E_RANGE, "%s: long rows without slots", who);
    a.HD = a.H * a.D, a.HK = a.H * a.K;
    if (EDGE) {
        if (int rc = dot_check_alias(who, {a.dq, a.dqe, a.pw, a.ds}, {a.q, a.k, a.v, a.qe, a.ef, a.dout, a.out, a.lse, a.aef, a.daef})) return rc;
    } else {
        if (int rc = dot_check_alias(who, {a.dq}, {a.q, a.k, a.v, a.dout, a.out})) return rc;
    }
    BOT_REQUIRE(a.pw != a.ds || nnz == 0, BOT_E_RANGE, "%s: p and ds alias each other", who);
    BOT_REQUIRE(!a.dq || a.dq != a.dqe, BOT_E_RANGE, "%s: dq and dqe alias each other", who);
    if (int rc = dot_check_strides(who, {{"ldq", a.ldq, a.HD}, {"ldk", a.ldk, a.HD}, {"ldv", a.ldv, a.HD}, {"ldd", a.ldd, a.HD}, {"ldo", a.ldo, a.HD},
                                         {"ldl", a.ldl, a.H}, {"lddq", a.dq ? a.lddq : a.HD, a.HD}, {"ldqe", a.ldqe, a.HK}, {"ldae", a.ldae, a.HK},
                                         {"lddae", a.lddae, a.HK}, {"lddqe", a.dqe ? a.lddqe : a.HK, a.HK}, {"ldef", a.ldef, a.K}}))
        return rc;
    if (int rc = dot_check_aligned(who, {a.q, a.k, a.v, a.qe, a.ef, a.dout, a.out, a.lse, a.aef, a.daef, a.pw, a.ds, a.dq, a.dqe, a.keep}, a.items,
                                   a.partial))
        return rc;
    int vec = pick_vec(a.D, {a.ldq, a.ldk, a.ldv, a.ldd, a.ldo, a.dq ? a.lddq : 0}, {a.q, a.k, a.v, a.dout, a.out, a.dq});
    if (EDGE) vec = dot_edge_vec(vec, a.D, a.K);
    if (int rc = dot_check_head(who, a.D, vec)) return rc;
    a.c = a.keep ? 1.f / (1.f - p) : 1.f;
    if constexpr (EDGE) dot_dispatch<DotDstKern<false, true>>(a, vec, st);
    else if (a.k == a.v && a.ldk == a.ldv) dot_dispatch<DotDstKern<true, false>>(a, vec, st);
    else dot_dispatch<DotDstKern<false, false>>(a, vec, st);
    if (int rc = dot_status(who, "launch")) return rc;
    if (n_long > 0 && (a.dq || a.dqe)) {
        if (a.dq) launch_sum_combine(a.partial, a.HD, a.dq, a.lddq, long_rows, long_ptr, n_long, st);
        if (a.dqe) launch_sum_combine(a.partial + a.n_slots * a.HD, a.HK, a.dqe, a.lddqe, long_rows, long_ptr, n_long, st);
        if (int rc = dot_status(who, "combine launch")) return rc;
    }
    return 0;
}

}  // namespace bot

extern "C" {

int bot_dot_attn_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                     const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots, const float* q, int64_t ldq,
                     const float* k, int64_t ldk, const float* v, int64_t ldv, int32_t H, int32_t D, float scale, const int32_t* keep, float p,
                     float* out, int64_t ldo, float* lse, int64_t ldl, void* workspace, bot_stream_t stream) {
    using namespace bot;
    (void)indptr;
    DotFwdArgs a{};
    a.indices = indices, a.items = reinterpret_cast<const int4*>(items), a.n_items = n_items, a.H = H, a.D = D, a.scale = scale, a.keep = keep;
    a.q = q, a.ldq = ldq, a.k = k, a.ldk = ldk, a.v = v, a.ldv = ldv;
    a.out = out, a.ldo = ldo, a.lse = lse, a.ldl = ldl, a.ws = static_cast<float*>(workspace), a.n_slots = n_slots;
    return dot_forward<false>("dot_attn", a, n_rows, nnz, long_rows, long_ptr, n_long, p, (hipStream_t)stream);
}

int bot_dot_attn_edge_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                          const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots, const float* q, int64_t ldq,
                          const float* k, int64_t ldk, const float* v, int64_t ldv, const float* qe, int64_t ldqe, const float* ef, int64_t ldef,
                          int32_t H, int32_t D, int32_t K, float scale, const int32_t* keep, float p, float* out, int64_t ldo, float* lse,
                          int64_t ldl, float* aef, int64_t ldae, void* workspace, bot_stream_t stream) {
    using namespace bot;
    (void)indptr;
    DotFwdArgs a{};
    a.indices = indices, a.items = reinterpret_cast<const int4*>(items), a.n_items = n_items, a.H = H, a.D = D, a.scale = scale, a.keep = keep;
    a.q = q, a.ldq = ldq, a.k = k, a.ldk = ldk, a.v = v, a.ldv = ldv;
    a.out = out, a.ldo = ldo, a.lse = lse, a.ldl = ldl, a.ws = static_cast<float*>(workspace), a.n_slots = n_slots;
    a.qe = qe, a.ldqe = ldqe, a.ef = ef, a.ldef = ldef, a.K = K, a.aef = aef, a.ldae = ldae;
    return dot_forward<true>("dot_attn_edge", a, n_rows, nnz, long_rows, long_ptr, n_long, p, (hipStream_t)stream);
}

int bot_dot_attn_bwd_dst_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                             const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, const float* q, int64_t ldq, const float* k,
                             int64_t ldk, const float* v, int64_t ldv, int32_t H, int32_t D, float scale, const int32_t* keep, float p,
                             const float* dout, int64_t ldd, const float* out, int64_t ldo, const float* lse, int64_t ldl, float* pw, float* ds,
                             float* dq, int64_t lddq, float* partial, bot_stream_t stream) {
    using namespace bot;
    (void)indptr;
    DotDstArgs a{};
    a.indices = indices, a.items = reinterpret_cast<const int4*>(items), a.n_items = n_items, a.H = H, a.D = D, a.scale = scale, a.keep = keep;
    a.q = q, a.ldq = ldq, a.k = k, a.ldk = ldk, a.v = v, a.ldv = ldv;
    a.dout = dout, a.ldd = ldd, a.out = out, a.ldo = ldo, a.lse = lse, a.ldl = ldl;
    a.pw = pw, a.ds = ds, a.dq = dq, a.lddq = lddq, a.partial = partial;
    return dot_backward_dst<false>("dot_attn_bwd_dst", a, n_rows, nnz, long_rows, long_ptr, n_long, p, (hipStream_t)stream);
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
    DotDstArgs a{};
    a.indices = indices, a.items = reinterpret_cast<const int4*>(items), a.n_items = n_items, a.H = H, a.D = D, a.scale = scale, a.keep = keep;
    a.q = q, a.ldq = ldq, a.k = k, a.ldk = ldk, a.v = v, a.ldv = ldv;
    a.dout = dout, a.ldd = ldd, a.out = out, a.ldo = ldo, a.lse = lse, a.ldl = ldl;
    a.pw = pw, a.ds = ds, a.dq = dq, a.lddq = lddq, a.partial = partial;
    a.qe = qe, a.ldqe = ldqe, a.ef = ef, a.ldef = ldef, a.K = K, a.aef = aef, a.ldae = ldae, a.daef = daef, a.lddae = lddae;
    a.dqe = dqe, a.lddqe = lddqe, a.n_slots = n_slots;
    return dot_backward_dst<true>("dot_attn_edge_bwd_dst", a, n_rows, nnz, long_rows, long_ptr, n_long, p, (hipStream_t)stream);
}

int bot_dot_attn_bwd_src_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                             const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots, const int32_t* pos,
                             const float* q, int64_t ldq, const float* dout, int64_t ldd, const float* pw, const float* ds, int32_t H, int32_t D,
                             float scale, float* dk, int64_t lddk, float* dv, int64_t lddv, float* partial, bot_stream_t stream) {
    using namespace bot;
    (void)indptr;
    const char* who = "dot_attn_bwd_src";
    if (int rc = check_plan_sizes(who, n_rows, nnz, n_items, n_long, n_slots)) return rc;
    if (int rc = dot_check_common(who, H, D, scale, false, 0, nullptr, 0.f)) return rc;
    if (n_rows == 0 || (!dk && !dv)) return 0;
    if (int rc = check_plan(who, items, "items", true, nnz, "indices/pos/q/dout/p/ds", indices && pos && q && dout && pw && ds, n_long,
                       "long_rows/long_ptr/partial", long_rows && long_ptr && partial)) return rc;
    BOT_REQUIRE(n_long == 0 || n_slots > 0, BOT_E_RANGE, "%s: long rows without slots", who);
    const int32_t HD = H * D;
    if (int rc = dot_check_alias(who, {dk, dv}, {q, dout})) return rc;
    BOT_REQUIRE(dk != dv || lddk == lddv, BOT_E_RANGE, "%s: one output for dk + dv has one row stride", who);
    if (int rc = dot_check_strides(who, {{"ldq", ldq, HD}, {"ldd", ldd, HD}, {"lddk", dk ? lddk : HD, HD}, {"lddv", dv ? lddv : HD, HD}})) return rc;
    if (int rc = dot_check_aligned(who, {q, dout, pw, ds, dk, dv, pos}, items, partial)) return rc;
    const int vec = pick_vec(D, {ldq, ldd, dk ? lddk : 0, dv ? lddv : 0, n_slots * HD}, {q, dout, dk, dv});
    if (int rc = dot_check_head(who, D, vec)) return rc;
    hipStream_t st = (hipStream_t)stream;
    DotSrcArgs a{};
    a.indices = indices, a.pos = pos, a.items = reinterpret_cast<const int4*>(items), a.n_items = n_items;
    a.q = q, a.ldq = ldq, a.dout = dout, a.ldd = ldd, a.H = H, a.D = D, a.HD = HD, a.scale = scale;
    a.pw = pw, a.ds = ds, a.dk = dk, a.lddk = lddk, a.dv = dv, a.lddv = lddv;
    a.partial = partial, a.n_slots = n_slots;
    dot_dispatch<DotSrcKern>(a, vec, st);
    if (int rc = dot_status(who, "launch")) return rc;
    if (n_long > 0) {
        if (dk) launch_sum_combine(partial, HD, dk, lddk, long_rows, long_ptr, n_long, st);
        if (dv && dv != dk) launch_sum_combine(partial + n_slots * HD, HD, dv, lddv, long_rows, long_ptr, n_long, st);
        if (int rc = dot_status(who, "combine launch")) return rc;
    }
    return 0;
}

}  // extern "C"
