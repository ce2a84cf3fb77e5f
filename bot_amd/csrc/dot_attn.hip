// Dot-product attention over a node's in-edges (include/bot_gnn.h "Dot-product attention") for gfx950: the layer of UniMP (Shi et al.,
// "Masked Label Prediction", IJCAI 2021, arXiv:2009.03509), PyG's TransformerConv and DGL's DotGatConv (bot_amd.nn, `ops.dot_attention`).
// Per head h, with s_k = scale * sum_d q[v,h,d] k[u_k,h,d] over the in-edges k of v, keep_k,h in {0, 1} the attention-dropout mask and
// c = 1 / (1 - p):
//   forward        lse[v,h] = log sum_k exp(s_k),  a_k = exp(s_k - lse[v,h]),  out[v,h,:] = c sum_k keep_k a_k v[u_k,h,:]   (rows = destinations: CSC)
//                  an empty row gives out = 0, lse = 0
//   backward, dst  delta[v,h] = sum_d dout[v,h,d] out[v,h,d],  dd_k = sum_d dout[v,h,d] v[u_k,h,d],  p_k = c keep_k a_k,
//                  ds_k = a_k (c keep_k dd_k - delta[v,h]),  dq[v,h,:] = scale sum_k ds_k k[u_k,h,:];  stores p[k,h], ds[k,h]          (the CSC)
//   backward, src  dk[u,h,:] = scale sum_j ds[pos_j,h] q[v_j,h,:],  dv[u,h,:] = sum_j p[pos_j,h] dout[v_j,h,:]             (rows = sources: CSR)
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
// HBM model (4-byte words; HD = H*D): forward 4 [E (1 + 2 HD) + n_dst (2 HD + H)] (ids, a k and a v row per edge; q read, out and lse
// written per row), E (1 + HD) when k and v are shared; backward over destinations 4 [E (1 + 2 HD + 2 H) + n_dst (4 HD + 2 H)] (ids, k
// and v rows, p and ds written per edge; q, dout, out read, dq written, lse read per row; the keep word adds E); backward over sources
// 4 [E (2 + 2 HD + 2 H) + 3 n_src HD] (ids and positions, q and dout rows, p and ds per edge; dk and dv written per row).
#include "dot.h"

#include <cmath>
#include <initializer_list>

namespace bot {

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
    float* ws;  // S [n_slots, HD], M [n_slots, H], Z [n_slots, H]: the chunks' states of the long rows
    int64_t n_slots;
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
    float* partial;  // [n_slots, HD] chunk sums of the long rows
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

template <bool SHARED, int VEC, int NCHUNK>
struct DotStage {
    float k[NCHUNK][VEC];
    float v[SHARED ? 1 : NCHUNK][SHARED ? 1 : VEC];
    __device__ __forceinline__ float val(int c, int t) const {
        if constexpr (SHARED) return k[c][t];
        else return v[c][t];
    }
};

template <bool SHARED, int VEC, int LANES, int NCHUNK>
__global__ __launch_bounds__(kBlock) void dot_attn_kernel(DotFwdArgs a) {
    using Stage = DotStage<SHARED, VEC, NCHUNK>;
    constexpr int U = dot_unroll(NCHUNK * VEC * (SHARED ? 1 : 2));
    const int lane = threadIdx.x % LANES;
    const int64_t item = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / LANES;
    if (item >= a.n_items) return;  // whole groups leave together
    const RowItem it = load_item<LANES>(a.items, item);
    const int tcols = a.hpt * a.D;
    for (int col0 = 0; col0 < a.HD; col0 += tcols) {  // groups narrower than a wavefront have one tile (DotLaunch)
        const HeadTile<VEC, LANES, NCHUNK> ht(col0, min(a.HD, col0 + tcols), lane, a.D);
        float qv[NCHUNK][VEC], M[NCHUNK] = {}, Z[NCHUNK] = {}, S[NCHUNK][VEC] = {};
#pragma unroll
        for (int c = 0; c < NCHUNK; ++c) vload<VEC>(qv[c], a.q + (int64_t)it.row * a.ldq + ht.off[c]);
        walk_row<LANES, Stage, U>(
            it.beg, it.end, lane, [&](int k, bool in) { return Edge{in ? a.indices[k] : 0, in && a.keep ? a.keep[k] : -1}; },
            [&](int s, int, Stage& st) {
                const float* pk = a.k + (int64_t)s * a.ldk;
                const float* pv = a.v + (int64_t)s * a.ldv;
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c) {
                    vload<VEC>(st.k[c], pk + ht.off[c]);
                    if constexpr (!SHARED) vload<VEC>(st.v[c], pv + ht.off[c]);
                }
            },
            [&](int, int w, const Stage& st, int k) {
                float p[1][NCHUNK];
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c) {
                    p[0][c] = qv[c][0] * st.k[c][0];
#pragma unroll
                    for (int t = 1; t < VEC; ++t) p[0][c] += qv[c][t] * st.k[c][t];
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
                    M[c] = up ? s : M[c];
                }
            });
        if (it.slot >= 0) {  // a chunk of a long row: the raw state, folded by dot_attn_combine_kernel
            float* wS = a.ws + (int64_t)it.slot * a.HD;
            float* wM = a.ws + a.n_slots * a.HD + (int64_t)it.slot * a.H;
#pragma unroll
            for (int c = 0; c < NCHUNK; ++c) {
                if (ht.act[c]) vstore<VEC>(wS + ht.off[c], S[c]);
                if (ht.first[c]) {
                    wM[ht.hid[c]] = M[c];
                    wM[a.n_slots * a.H + ht.hid[c]] = Z[c];
                }
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
        }
    }
}

// One thread per (long row, column): the chunks' states are folded in slot order (= position order) with the sweep's merge, then the
// row's epilogue.  (A long row has at least two chunks and no chunk is empty.)
__global__ __launch_bounds__(kBlock) void dot_attn_combine_kernel(DotFwdArgs a, const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long) {
    const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gid >= n_long * a.HD) return;
    const int64_t i = gid / a.HD;
    const int col = (int)(gid - i * a.HD);
    const int h = col / a.D;
    const int row = long_rows[i], p1 = long_ptr[i + 1];
    int s = long_ptr[i];
    const float* wS = a.ws + col;
    const float* wM = a.ws + a.n_slots * a.HD + h;
    const float* wZ = wM + a.n_slots * a.H;
    float M = 0.f, Z = 0.f, S = 0.f, Q = 0.f;
    const bool some = s < p1;
    if (some) {
        M = wM[(int64_t)s * a.H], Z = wZ[(int64_t)s * a.H], S = wS[(int64_t)s * a.HD];
        ++s;
    }
    for (; s < p1; ++s) smx_merge<false>(M, Z, S, Q, wM[(int64_t)s * a.H], wZ[(int64_t)s * a.H], wS[(int64_t)s * a.HD], 0.f);
    a.out[(int64_t)row * a.ldo + col] = some ? a.c * (S / Z) : 0.f;
    if (col == h * a.D) a.lse[(int64_t)row * a.ldl + h] = some ? M + logf(Z) : 0.f;
}

template <bool SHARED, int VEC, int LANES, int NCHUNK>
__global__ __launch_bounds__(kBlock) void dot_attn_bwd_dst_kernel(DotDstArgs a) {
    using Stage = DotStage<SHARED, VEC, NCHUNK>;
    constexpr int U = dot_unroll(NCHUNK * VEC * (SHARED ? 1 : 2));
    const int lane = threadIdx.x % LANES;
    const int64_t item = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / LANES;
    if (item >= a.n_items) return;  // whole groups leave together
    const RowItem it = load_item<LANES>(a.items, item);
    const int tcols = a.hpt * a.D;
    for (int col0 = 0; col0 < a.HD; col0 += tcols) {
        const HeadTile<VEC, LANES, NCHUNK> ht(col0, min(a.HD, col0 + tcols), lane, a.D);
        float qv[NCHUNK][VEC], dv[NCHUNK][VEC], acc[NCHUNK][VEC] = {}, delta[1][NCHUNK], lse[NCHUNK];
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
        }
        ht.template total<1>(delta);
        walk_row<LANES, Stage, U>(
            it.beg, it.end, lane, [&](int k, bool in) { return Edge{in ? a.indices[k] : 0, in && a.keep ? a.keep[k] : -1}; },
            [&](int s, int, Stage& st) {
                const float* pk = a.k + (int64_t)s * a.ldk;
                const float* pv = a.v + (int64_t)s * a.ldv;
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c) {
                    vload<VEC>(st.k[c], pk + ht.off[c]);
                    if constexpr (!SHARED) vload<VEC>(st.v[c], pv + ht.off[c]);
                }
            },
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
                }
                ht.template total<2>(p);
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c) {
                    const float w_a = smx_exp(a.scale * p[0][c] - lse[c]);
                    const float ck = dot_kept(w, ht.hid[c]) ? a.c : 0.f;
                    const float g = w_a * (ck * p[1][c] - delta[0][c]);
#pragma unroll
                    for (int t = 0; t < VEC; ++t) acc[c][t] = fmaf(g, st.k[c][t], acc[c][t]);
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
            [&](int s, int w, Stage& st) {
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

template <bool SHARED>
struct DotFwdKern {
    template <int VEC, int LANES, int NCHUNK>
    static void launch(const DotFwdArgs& b, unsigned blocks, hipStream_t st) {
        set_kernel("bot::dot_attn_kernel<%d,%d,%d,%d>", (int)SHARED, VEC, LANES, NCHUNK);
        hipLaunchKernelGGL((dot_attn_kernel<SHARED, VEC, LANES, NCHUNK>), dim3(blocks), dim3(kBlock), 0, st, b);
    }
};
template <bool SHARED>
struct DotDstKern {
    template <int VEC, int LANES, int NCHUNK>
    static void launch(const DotDstArgs& b, unsigned blocks, hipStream_t st) {
        set_kernel("bot::dot_attn_bwd_dst_kernel<%d,%d,%d,%d>", (int)SHARED, VEC, LANES, NCHUNK);
        hipLaunchKernelGGL((dot_attn_bwd_dst_kernel<SHARED, VEC, LANES, NCHUNK>), dim3(blocks), dim3(kBlock), 0, st, b);
    }
};
struct DotSrcKern {
    template <int VEC, int LANES, int NCHUNK>
    static void launch(const DotSrcArgs& b, unsigned blocks, hipStream_t st) {
        set_kernel("bot::dot_attn_bwd_src_kernel<%d,%d,%d>", VEC, LANES, NCHUNK);
        hipLaunchKernelGGL((dot_attn_bwd_src_kernel<VEC, LANES, NCHUNK>), dim3(blocks), dim3(kBlock), 0, st, b);
    }
};

}  // namespace bot

extern "C" {

#define DOT_COMMON(name)                                                                                                       \
    BOT_REQUIRE(H >= 1 && D >= 1 && (int64_t)H * D < (1 << 24), BOT_E_RANGE, name ": H=%d D=%d (>= 1, H*D < 2^24)", H, D);  \
    BOT_REQUIRE(scale == scale, BOT_E_RANGE, name ": scale is NaN");

#define DOT_KEEP(name)                                                                                                         \
    BOT_REQUIRE(p >= 0.f && p < 1.f, BOT_E_RANGE, name ": p=%g (0 <= p < 1)", (double)p);                                   \
    BOT_REQUIRE(!keep || H <= 32, BOT_E_RANGE, name ": a keep mask holds one bit per head, H=%d (<= 32)", H);

int bot_dot_attn_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                     const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots, const float* q, int64_t ldq,
                     const float* k, int64_t ldk, const float* v, int64_t ldv, int32_t H, int32_t D, float scale, const int32_t* keep, float p,
                     float* out, int64_t ldo, float* lse, int64_t ldl, void* workspace, bot_stream_t stream) {
    using namespace bot;
    (void)indptr;
    if (int rc = check_plan_sizes("dot_attn", n_rows, nnz, n_items, n_long, n_slots)) return rc;
    DOT_COMMON("dot_attn")
    DOT_KEEP("dot_attn")
    if (n_rows == 0) return 0;
    if (int rc = check_plan("dot_attn", items, "items/q/out/lse", q && out && lse, nnz, "indices/k/v", indices && k && v, n_long,
                            "long_rows/long_ptr/workspace", long_rows && long_ptr && workspace))
        return rc;
    BOT_REQUIRE(n_long == 0 || n_slots > 0, BOT_E_RANGE, "dot_attn: long rows without slots");
    const int32_t HD = H * D;
    BOT_REQUIRE(out != q && out != k && out != v && lse != q && lse != k && lse != v && out != lse, BOT_E_RANGE,
                "dot_attn: out and lse alias an input or each other");
    BOT_REQUIRE(ldq >= HD && ldk >= HD && ldv >= HD && ldo >= HD && ldl >= H, BOT_E_RANGE,
                "dot_attn: row strides smaller than the rows (ldq=%lld ldk=%lld ldv=%lld ldo=%lld H*D=%d ldl=%lld H=%d)", (long long)ldq,
                (long long)ldk, (long long)ldv, (long long)ldo, HD, (long long)ldl, H);
    BOT_REQUIRE(aligned(q, 4) && aligned(k, 4) && aligned(v, 4) && aligned(out, 4) && aligned(lse, 4) && aligned(keep, 4) && aligned(items, 16) &&
                    aligned(workspace, 16),
                BOT_E_ALIGN, "dot_attn: misaligned pointer");
    const int vec = pick_vec(D, {ldq, ldk, ldv, ldo}, {q, k, v, out});
    BOT_REQUIRE(dot_head_fits(D, vec), BOT_E_RANGE, "dot_attn: a head of D=%d columns read %d at a time does not fit one tile of %d lanes", D,
                vec, kWave * kDotMaxChunk);
    hipStream_t st = (hipStream_t)stream;
    DotFwdArgs a{};
    a.indices = indices, a.keep = keep, a.items = reinterpret_cast<const int4*>(items), a.n_items = n_items;
    a.q = q, a.ldq = ldq, a.k = k, a.ldk = ldk, a.v = v, a.ldv = ldv, a.H = H, a.D = D, a.HD = HD;
    a.scale = scale, a.c = keep ? 1.f / (1.f - p) : 1.f;
    a.out = out, a.ldo = ldo, a.lse = lse, a.ldl = ldl, a.ws = static_cast<float*>(workspace), a.n_slots = n_slots;
    // (the workspace: 16-byte base, S rows of H*D floats first - H*D % vec == 0 keeps every row aligned - then M and Z)
    if (k == v && ldk == ldv) dot_dispatch<DotFwdKern<true>>(a, vec, st);
    else dot_dispatch<DotFwdKern<false>>(a, vec, st);
    if (int rc = hip_status("dot_attn launch")) return rc;
    if (n_long > 0) {
        hipLaunchKernelGGL(dot_attn_combine_kernel, dim3((unsigned)((n_long * HD + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, a, long_rows,
                           long_ptr, n_long);
        if (int rc = hip_status("dot_attn combine launch")) return rc;
    }
    return 0;
}

int bot_dot_attn_bwd_dst_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                             const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, const float* q, int64_t ldq, const float* k,
                             int64_t ldk, const float* v, int64_t ldv, int32_t H, int32_t D, float scale, const int32_t* keep, float p,
                             const float* dout, int64_t ldd, const float* out, int64_t ldo, const float* lse, int64_t ldl, float* pw, float* ds,
                             float* dq, int64_t lddq, float* partial, bot_stream_t stream) {
    using namespace bot;
    (void)indptr;
    if (int rc = check_plan_sizes("dot_attn_bwd_dst", n_rows, nnz, n_items, n_long)) return rc;
    DOT_COMMON("dot_attn_bwd_dst")
    DOT_KEEP("dot_attn_bwd_dst")
    if (n_rows == 0) return 0;
    if (int rc = check_plan("dot_attn_bwd_dst", items, "items/q/dout/out/lse", q && dout && out && lse, nnz, "indices/k/v/p/ds",
                            indices && k && v && pw && ds, n_long && dq, "long_rows/long_ptr/partial", long_rows && long_ptr && partial))
        return rc;
    const int32_t HD = H * D;
    BOT_REQUIRE(!dq || (dq != q && dq != k && dq != v && dq != dout && dq != out), BOT_E_RANGE, "dot_attn_bwd_dst: dq aliases an input");
    BOT_REQUIRE(pw != ds || nnz == 0, BOT_E_RANGE, "dot_attn_bwd_dst: p and ds alias each other");
    BOT_REQUIRE(ldq >= HD && ldk >= HD && ldv >= HD && ldd >= HD && ldo >= HD && ldl >= H && (!dq || lddq >= HD), BOT_E_RANGE,
                "dot_attn_bwd_dst: row strides smaller than the rows (ldq=%lld ldk=%lld ldv=%lld ldd=%lld ldo=%lld lddq=%lld H*D=%d ldl=%lld H=%d)",
                (long long)ldq, (long long)ldk, (long long)ldv, (long long)ldd, (long long)ldo, (long long)lddq, HD, (long long)ldl, H);
    BOT_REQUIRE(aligned(q, 4) && aligned(k, 4) && aligned(v, 4) && aligned(dout, 4) && aligned(out, 4) && aligned(lse, 4) && aligned(pw, 4) &&
                    aligned(ds, 4) && aligned(dq, 4) && aligned(keep, 4) && aligned(items, 16) && aligned(partial, 16),
                BOT_E_ALIGN, "dot_attn_bwd_dst: misaligned pointer");
    const int vec = pick_vec(D, {ldq, ldk, ldv, ldd, ldo, dq ? lddq : 0}, {q, k, v, dout, out, dq});
    BOT_REQUIRE(dot_head_fits(D, vec), BOT_E_RANGE, "dot_attn_bwd_dst: a head of D=%d columns read %d at a time does not fit one tile of %d lanes",
                D, vec, kWave * kDotMaxChunk);
    hipStream_t st = (hipStream_t)stream;
    DotDstArgs a{};
    a.indices = indices, a.keep = keep, a.items = reinterpret_cast<const int4*>(items), a.n_items = n_items;
    a.q = q, a.ldq = ldq, a.k = k, a.ldk = ldk, a.v = v, a.ldv = ldv, a.H = H, a.D = D, a.HD = HD;
    a.scale = scale, a.c = keep ? 1.f / (1.f - p) : 1.f;
    a.dout = dout, a.ldd = ldd, a.out = out, a.ldo = ldo, a.lse = lse, a.ldl = ldl;
    a.pw = pw, a.ds = ds, a.dq = dq, a.lddq = lddq, a.partial = partial;
    if (k == v && ldk == ldv) dot_dispatch<DotDstKern<true>>(a, vec, st);
    else dot_dispatch<DotDstKern<false>>(a, vec, st);
    if (int rc = hip_status("dot_attn_bwd_dst launch")) return rc;
    if (dq && n_long > 0) {
        launch_sum_combine(partial, HD, dq, lddq, long_rows, long_ptr, n_long, st);
        if (int rc = hip_status("dot_attn_bwd_dst combine launch")) return rc;
    }
    return 0;
}

int bot_dot_attn_bwd_src_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                             const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots, const int32_t* pos,
                             const float* q, int64_t ldq, const float* dout, int64_t ldd, const float* pw, const float* ds, int32_t H, int32_t D,
                             float scale, float* dk, int64_t lddk, float* dv, int64_t lddv, float* partial, bot_stream_t stream) {
    using namespace bot;
    (void)indptr;
    if (int rc = check_plan_sizes("dot_attn_bwd_src", n_rows, nnz, n_items, n_long, n_slots)) return rc;
    DOT_COMMON("dot_attn_bwd_src")
    if (n_rows == 0 || (!dk && !dv)) return 0;
    if (int rc = check_plan("dot_attn_bwd_src", items, "items", true, nnz, "indices/pos/q/dout/p/ds", indices && pos && q && dout && pw && ds, n_long,
                            "long_rows/long_ptr/partial", long_rows && long_ptr && partial))
        return rc;
    BOT_REQUIRE(n_long == 0 || n_slots > 0, BOT_E_RANGE, "dot_attn_bwd_src: long rows without slots");
    const int32_t HD = H * D;
    BOT_REQUIRE(dk != q && dk != dout && dv != q && dv != dout, BOT_E_RANGE, "dot_attn_bwd_src: dk / dv aliases an input");
    BOT_REQUIRE(dk != dv || lddk == lddv, BOT_E_RANGE, "dot_attn_bwd_src: one output for dk + dv has one row stride");
    BOT_REQUIRE(ldq >= HD && ldd >= HD && (!dk || lddk >= HD) && (!dv || lddv >= HD), BOT_E_RANGE,
                "dot_attn_bwd_src: row strides smaller than the rows (ldq=%lld ldd=%lld lddk=%lld lddv=%lld H*D=%d)", (long long)ldq, (long long)ldd,
                (long long)lddk, (long long)lddv, HD);
    BOT_REQUIRE(aligned(q, 4) && aligned(dout, 4) && aligned(pw, 4) && aligned(ds, 4) && aligned(dk, 4) && aligned(dv, 4) && aligned(pos, 4) &&
                    aligned(items, 16) && aligned(partial, 16),
                BOT_E_ALIGN, "dot_attn_bwd_src: misaligned pointer");
    const int vec = pick_vec(D, {ldq, ldd, dk ? lddk : 0, dv ? lddv : 0, n_slots * HD}, {q, dout, dk, dv});
    BOT_REQUIRE(dot_head_fits(D, vec), BOT_E_RANGE, "dot_attn_bwd_src: a head of D=%d columns read %d at a time does not fit one tile of %d lanes",
                D, vec, kWave * kDotMaxChunk);
    hipStream_t st = (hipStream_t)stream;
    DotSrcArgs a{};
    a.indices = indices, a.pos = pos, a.items = reinterpret_cast<const int4*>(items), a.n_items = n_items;
    a.q = q, a.ldq = ldq, a.dout = dout, a.ldd = ldd, a.H = H, a.D = D, a.HD = HD, a.scale = scale;
    a.pw = pw, a.ds = ds, a.dk = dk, a.lddk = lddk, a.dv = dv, a.lddv = lddv;
    a.partial = partial, a.n_slots = n_slots;
    dot_dispatch<DotSrcKern>(a, vec, st);
    if (int rc = hip_status("dot_attn_bwd_src launch")) return rc;
    if (n_long > 0) {
        if (dk) launch_sum_combine(partial, HD, dk, lddk, long_rows, long_ptr, n_long, st);
        if (dv && dv != dk) launch_sum_combine(partial + n_slots * HD, HD, dv, lddv, long_rows, long_ptr, n_long, st);
        if (int rc = hip_status("dot_attn_bwd_src combine launch")) return rc;
    }
    return 0;
}

}  // extern "C"
