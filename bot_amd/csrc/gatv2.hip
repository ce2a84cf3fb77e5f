// GATv2 edge logits (include/bot_gnn.h "GATv2 edge logits") for gfx950: the score of Brody, Alon, Yahav, "How Attentive are Graph Attention
// Networks?" (ICLR 2022; bot_amd.nn.GATv2Conv), whose nonlinearity sits INSIDE the dot product, so it does not split into per-node scalars:
//   forward        e[k,h]   = sum_d attn[h,d] * lrelu(fs[u_k,h,d] + fd[v_k,h,d])                      (rows = destinations: the CSC)
//   backward, dst  dfd[v]   = sum over the in-edges k of v of t[k],  t[k,h,d] = de[k,h] * attn[h,d] * lrelu'(s)            (the CSC)
//                  dattn    = sum over all k of de[k,h] * lrelu(s[k,h,d])                             (a by-product of the same pass)
//   backward, src  dfs[u]   = sum over the out-edges j of u of t[pos(j)]                               (rows = sources: the CSR)
// with s = fs[u,h,d] + fd[v,h,d], lrelu(s) = s > 0 ? s : slope * s and lrelu'(s) = s > 0 ? 1 : slope (torch's convention at s == 0).
//
// The gather is the lane-group row sweep that sweep.h describes, over the H*D columns (VEC divides D, so a lane's vector never straddles two
// heads).  A row wider than the group's tile (64 lanes x VEC x NCHUNK, NCHUNK up to 6: H*D = 750 is one tile of 8-byte lanes) walks feature
// tiles; the ids are read again per tile.
// The row a group owns (fd of the destination, fs of the source) and attn stay in registers across its neighbours.  Two dependent load
// levels: the ids (with them the edge's output / de position), then the rows - which wait on nothing but indices[k].
//
// Forward: per neighbour the fused add / lrelu / multiply, then a SEGMENTED scan over the lanes of each 64-lane chunk (log2 LANES shuffle
// steps, each lane adding the value 2^s lanes below it while that lane is of its head; steps that join nothing anywhere in the wavefront
// are skipped), so a head may be a fraction of a group, a whole group, or span chunks: the last lane of a chunk hands its sum to lane 0 of
// the next one.  The last lane of a head stores e[k,h] once.  A head that spans feature TILES leaves its partial sum in e[k,h] and the
// next tile's last lane of that head adds to it (same wavefront, program order; tiles in ascending order), so the order of the sum over d
// is fixed per (k, h).  Long rows need no combine: the outputs are per edge.
//
// Backward over destinations: the same gather with de[k, head of the column] read beside the ids' level.  dfd[v] is a row-owner sum in
// registers, long rows chunk by chunk into `partial` and through the slot-order combine.  The kernel is persistent (a grid of at most
// kMaxGrid workgroups, items dealt round-robin to the groups) so that the dattn partials are bounded by the grid, not by E: every lane
// keeps the dattn sums of its columns in registers over all its items, the groups of a workgroup are folded in group order through LDS
// into one row of the [n_partials, H*D] workspace, and gatv2_dattn_reduce_kernel (one wavefront per column: rows lane, lane + 64, ... in
// order, then the butterfly) finishes.  Backward over sources: fs[u] in registers, per out-edge the destination's fd row and de through
// `pos` (Graph.csr2csc), dfs[u] a row-owner sum with the same combine.  No float atomics anywhere: all three repeat their bytes.
//
// HBM model (4-byte words; HD = H*D): forward 4 [E (1 + HD + H) + n_dst HD] (ids, a source row and the H outputs per edge; fd per row);
// backward over destinations 4 [E (1 + HD + H) + 2 n_dst HD] (ids, a source row, de per edge; fd read and dfd written per row);
// backward over sources 4 [E (2 + HD + H) + 2 n_src HD] (ids and positions, a destination row, de per edge; fs read and dfs written).
#include "sweep.h"

#include <initializer_list>

namespace bot {

constexpr int kGv2MaxGrid = 2048;  // workgroups of the persistent backward: the bound of the dattn partials

struct Gv2Args {
    const int32_t* indices;
    const int32_t* perm;  // forward: e's row of position k (NULL: k); backward dst: de's row of position k (NULL: k); backward src: de's row of position j
    const int4* items;
    int64_t n_items;
    const float* fs;
    int64_t ldfs;
    const float* fd;
    int64_t ldfd;
    const float* attn;
    int32_t D, HD;
    float slope;
    float* e;  // forward: the output; backward: de (read only)
    int64_t lde;
    float* out;  // backward: dfd / dfs (NULL: not asked for)
    int64_t ldo;
    float* partial;  // [n_slots, HD] chunk sums of the long rows
    float* dpart;    // [gridDim.x, HD] dattn partials (NULL: not asked for)
};

__device__ __forceinline__ float lrelu(float s, float slope) { return s > 0.f ? s : slope * s; }

template <int LANES>
__device__ __forceinline__ constexpr int log2_lanes() {
    return LANES == 64 ? 6 : LANES == 32 ? 5 : LANES == 16 ? 4 : 3;
}

template <int VEC, int LANES, int NCHUNK>
__global__ __launch_bounds__(kBlock) void gatv2_logits_kernel(Gv2Args a) {
    constexpr int TILE = LANES * VEC * NCHUNK;
    constexpr int STEPS = log2_lanes<LANES>();
    const int lane = threadIdx.x % LANES;
    const int64_t item = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / LANES;
    if (item >= a.n_items) return;  // whole groups leave together
    const RowItem it = load_item<LANES>(a.items, item);
    for (int col0 = 0; col0 < a.HD; col0 += TILE) {  // groups narrower than a wavefront have one tile (Gv2Launch)
        int off[NCHUNK], hid[NCHUNK];
        unsigned join[NCHUNK], anyjoin[NCHUNK];
        bool last[NCHUNK], rmw[NCHUNK], take[NCHUNK];
        float fdv[NCHUNK][VEC], at[NCHUNK][VEC];
#pragma unroll
        for (int c = 0; c < NCHUNK; ++c) {
            const int e = col0 + (c * LANES + lane) * VEC;
            const bool act = e < a.HD;
            off[c] = act ? e : 0;            // idle lanes re-read column 0: always in bounds, never stored
            hid[c] = act ? e / a.D : -1;     // ... and are a segment of their own
            vload<VEC>(fdv[c], a.fd + (int64_t)it.row * a.ldfd + off[c]);
            vload<VEC>(at[c], a.attn + off[c]);
        }
#pragma unroll
        for (int c = 0; c < NCHUNK; ++c) {
            join[c] = anyjoin[c] = 0u;
#pragma unroll
            for (int s = 0; s < STEPS; ++s) {
                const int below = __shfl_up(hid[c], 1 << s, LANES);
                const bool j = lane >= (1 << s) && below == hid[c];
                join[c] |= j ? 1u << s : 0u;
                anyjoin[c] |= __ballot(j) != 0 ? 1u << s : 0u;  // wave-uniform
            }
            const int above = __shfl_down(hid[c], 1, LANES);
            int next = -2;
            if (c + 1 < NCHUNK) next = group_bcast<LANES>(hid[c + 1 < NCHUNK ? c + 1 : c], 0);
            const int nxt = lane == LANES - 1 ? next : above;
            last[c] = hid[c] >= 0 && nxt != hid[c];
            rmw[c] = last[c] && hid[c] * a.D < col0;  // the head began in an earlier tile: add to what that tile left
            take[c] = false;
            if (c > 0) take[c] = lane == 0 && hid[c] >= 0 && group_bcast<LANES>(hid[c > 0 ? c - 1 : 0], LANES - 1) == hid[c];
        }
        // one neighbour: v holds its gathered row, o the row of e it writes
        auto edge = [&](const float (&v)[NCHUNK][VEC], int64_t o) {
            float p[NCHUNK];
#pragma unroll
            for (int c = 0; c < NCHUNK; ++c) {
                p[c] = 0.f;
#pragma unroll
                for (int t = 0; t < VEC; ++t) p[c] += at[c][t] * lrelu(v[c][t] + fdv[c][t], a.slope);
            }
#pragma unroll
            for (int c = 0; c < NCHUNK; ++c) {
                if (c > 0) {
                    const float tail = group_bcast<LANES>(p[c > 0 ? c - 1 : 0], LANES - 1);
                    if (take[c]) p[c] += tail;
                }
#pragma unroll
                for (int s = 0; s < STEPS; ++s)
                    if (anyjoin[c] >> s & 1u) {
                        const float below = __shfl_up(p[c], 1 << s, LANES);
                        if (join[c] >> s & 1u) p[c] += below;
                    }
                if (last[c]) {
                    float* q = a.e + o * a.lde + hid[c];
                    *q = rmw[c] ? *q + p[c] : p[c];
                }
            }
        };
        walk_row<LANES, float[NCHUNK][VEC]>(
            it.beg, it.end, lane,
            [&](int k, bool in) { return in ? Edge{a.indices[k], a.perm ? a.perm[k] : k} : Edge{0, 0}; },  // the word: e's row of position k
            [&](int s, int, float (&v)[NCHUNK][VEC], int) {
                const float* p = a.fs + (int64_t)s * a.ldfs;
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c) vload<VEC>(v[c], p + off[c]);
            },
            [&](int, int o, const float (&v)[NCHUNK][VEC], int) { edge(v, (int64_t)o); });
        // the next tile's lanes read what this tile's lanes stored (heads that span tiles): same wavefront, program order
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
}

// The two backward sweeps.  DST: rows = destinations, `own` = fd, gathered = fs, de's row of position k is perm[k] (or k); also the dattn
// partials.  !DST: rows = sources, `own` = fs, gathered = fd, de's row of position j is perm[j].
template <bool DST, int VEC, int LANES, int NCHUNK>
__global__ __launch_bounds__(kBlock) void gatv2_logits_bwd_kernel(Gv2Args a) {
    constexpr int U = 4;
    constexpr int TILE = LANES * VEC * NCHUNK;
    constexpr int GROUPS = kBlock / LANES;
    __shared__ float fold[DST ? kBlock * NCHUNK * VEC : 1];
    const int lane = threadIdx.x % LANES;
    const int group = threadIdx.x / LANES;
    const float* own = DST ? a.fd : a.fs;
    const int64_t ldown = DST ? a.ldfd : a.ldfs;
    const float* oth = DST ? a.fs : a.fd;
    const int64_t ldoth = DST ? a.ldfs : a.ldfd;
    const float* de = a.e;
    for (int col0 = 0; col0 < a.HD; col0 += TILE) {
        int off[NCHUNK], hid[NCHUNK];
        bool act[NCHUNK];
        float at[NCHUNK][VEC], da[NCHUNK][VEC];
#pragma unroll
        for (int c = 0; c < NCHUNK; ++c) {
            const int e = col0 + (c * LANES + lane) * VEC;
            act[c] = e < a.HD;
            off[c] = act[c] ? e : 0;  // idle lanes re-read column 0: always in bounds, never stored
            hid[c] = off[c] / a.D;
            vload<VEC>(at[c], a.attn + off[c]);
#pragma unroll
            for (int t = 0; t < VEC; ++t) da[c][t] = 0.f;
        }
        // items are dealt round-robin to the groups of the (persistent) grid
        for (int64_t item = (int64_t)blockIdx.x * GROUPS + group; item < a.n_items; item += (int64_t)gridDim.x * GROUPS) {
            const RowItem it = load_item<LANES>(a.items, item);
            float ov[NCHUNK][VEC], acc[NCHUNK][VEC];
#pragma unroll
            for (int c = 0; c < NCHUNK; ++c) {
                vload<VEC>(ov[c], own + (int64_t)it.row * ldown + off[c]);
#pragma unroll
                for (int t = 0; t < VEC; ++t) acc[c][t] = 0.f;
            }
            auto edge = [&](const float (&v)[NCHUNK][VEC], const float (&g)[NCHUNK]) {
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c)
#pragma unroll
                    for (int t = 0; t < VEC; ++t) {
                        const float s = v[c][t] + ov[c][t];
                        const bool pos = s > 0.f;
                        acc[c][t] += g[c] * at[c][t] * (pos ? 1.f : a.slope);
                        if constexpr (DST) da[c][t] += g[c] * (pos ? s : a.slope * s);
                    }
            };
            for (int k0 = it.beg; k0 < it.end; k0 += LANES) {
                const int k = k0 + lane;
                int idx = 0, dk = 0;
                if (k < it.end) {
                    idx = a.indices[k];
                    dk = a.perm ? a.perm[k] : k;
                }
                const int cnt = min(LANES, it.end - k0);
                int i = 0;
                for (; i + U <= cnt; i += U) {
                    float v[U][NCHUNK][VEC], g[U][NCHUNK];
#pragma unroll
                    for (int u = 0; u < U; ++u) {
                        const int s = group_bcast<LANES>(idx, i + u);
                        const float* p = oth + (int64_t)s * ldoth;
                        const float* q = de + (int64_t)group_bcast<LANES>(dk, i + u) * a.lde;
#pragma unroll
                        for (int c = 0; c < NCHUNK; ++c) {
                            vload<VEC>(v[u][c], p + off[c]);
                            g[u][c] = q[hid[c]];
                        }
                    }
#pragma unroll
                    for (int u = 0; u < U; ++u) edge(v[u], g[u]);
                }
                for (; i < cnt; ++i) {
                    const int s = group_bcast<LANES>(idx, i);
                    const float* p = oth + (int64_t)s * ldoth;
                    const float* q = de + (int64_t)group_bcast<LANES>(dk, i) * a.lde;
                    float v[NCHUNK][VEC], g[NCHUNK];
#pragma unroll
                    for (int c = 0; c < NCHUNK; ++c) {
                        vload<VEC>(v[c], p + off[c]);
                        g[c] = q[hid[c]];
                    }
                    edge(v, g);
                }
            }
            if (a.out) {
                float* po = sum_row(it, a.out, a.ldo, a.partial, a.HD);
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c)
                    if (act[c]) vstore<VEC>(po + off[c], acc[c]);
            }
        }
        if constexpr (DST) {
            if (a.dpart) {  // (uniform over the workgroup: every thread runs every tile)
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c)
#pragma unroll
                    for (int t = 0; t < VEC; ++t) fold[(c * VEC + t) * kBlock + threadIdx.x] = da[c][t];
                __syncthreads();
                if (group == 0) {
#pragma unroll
                    for (int c = 0; c < NCHUNK; ++c) {
                        float s[VEC];
#pragma unroll
                        for (int t = 0; t < VEC; ++t) {
                            s[t] = 0.f;
                            for (int gg = 0; gg < GROUPS; ++gg) s[t] += fold[(c * VEC + t) * kBlock + gg * LANES + lane];  // group order
                        }
                        if (act[c]) vstore<VEC>(a.dpart + (int64_t)blockIdx.x * a.HD + off[c], s);
                    }
                }
                __syncthreads();  // the next tile writes `fold` again
            }
        }
    }
}

// One wavefront per column of the [n_part, HD] dattn partials: lane l adds rows l, l + 64, ... in order, then the butterfly.
__global__ __launch_bounds__(kBlock) void gatv2_dattn_reduce_kernel(const float* dpart, int32_t n_part, int32_t HD, float* dattn) {
    const int col = (int)(((int64_t)blockIdx.x * kBlock + threadIdx.x) / kWave);
    const int lane = threadIdx.x % kWave;
    if (col >= HD) return;  // whole wavefronts leave together
    float s = 0.f;
    for (int r = lane; r < n_part; r += kWave) s += dpart[(int64_t)r * HD + col];
    s = group_sum<kWave>(s);
    if (lane == 0) dattn[col] = s;
}

enum Gv2Kind { GV2_FWD, GV2_BWD_DST, GV2_BWD_SRC };

// Workgroups of one launch: one group per item, the persistent backward over destinations capped at kGv2MaxGrid.
static int64_t gv2_grid(int kind, int64_t n_items, int lanes) {
    const int64_t blocks = (n_items * lanes + kBlock - 1) / kBlock;
    return kind == GV2_BWD_DST && blocks > kGv2MaxGrid ? kGv2MaxGrid : blocks;
}

template <int KIND>
struct Gv2Launch {
    const Gv2Args& a;
    hipStream_t st;
    // returns the workgroups of the launch
    template <int VEC, int LANES, int NCHUNK>
    int64_t run() const {
        const int64_t blocks = gv2_grid(KIND, a.n_items, LANES);
        if (blocks == 0) return 0;
        if constexpr (KIND == GV2_FWD) {
            set_kernel("bot::gatv2_logits_kernel<%d,%d,%d>", VEC, LANES, NCHUNK);
            hipLaunchKernelGGL((gatv2_logits_kernel<VEC, LANES, NCHUNK>), dim3((unsigned)blocks), dim3(kBlock), 0, st, a);
        } else {
            set_kernel("bot::gatv2_logits_bwd_kernel<%d,%d,%d,%d>", (int)(KIND == GV2_BWD_DST), VEC, LANES, NCHUNK);
            hipLaunchKernelGGL((gatv2_logits_bwd_kernel<KIND == GV2_BWD_DST, VEC, LANES, NCHUNK>), dim3((unsigned)blocks), dim3(kBlock), 0, st, a);
        }
        return blocks;
    }
    template <int VEC>
    int64_t wide(int L) const {
        if (L <= 128) return run<VEC, 64, 2>();
        if (L > 256 && L <= 384) return run<VEC, 64, 6>();  // H*D = 750 with 8-byte lanes: one tile
        return run<VEC, 64, 4>();                           // wider rows walk tiles of 256 lanes
    }
};

// The largest grid the backward over destinations may take (LANES = 64): the workspace's bound on the dattn partials.
static int64_t gv2_max_partials(int64_t n_items) { return gv2_grid(GV2_BWD_DST, n_items, kWave); }

}  // namespace bot

extern "C" {

#define GV2_COMMON(name)                                                                                                                   \
    if (int rc = check_plan_sizes(name, n_rows, nnz, n_items)) return rc;                                                                \
    BOT_REQUIRE(H >= 1 && D >= 1 && (int64_t)H * D < (1 << 24), BOT_E_RANGE, name ": H=%d D=%d (>= 1, H*D < 2^24)", H, D);              \
    BOT_REQUIRE(slope == slope, BOT_E_RANGE, name ": slope is NaN");

int bot_gatv2_logits_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                         const float* fs, int64_t ldfs, const float* fd, int64_t ldfd, const float* attn, int32_t H, int32_t D, float slope,
                         const int32_t* operm, float* e, int64_t lde, bot_stream_t stream) {
    using namespace bot;
    (void)indptr;
    GV2_COMMON("gatv2_logits")
    if (n_rows == 0 || nnz == 0) return 0;
    const int32_t HD = H * D;
    BOT_REQUIRE(items && indices && fs && fd && attn && e, BOT_E_NULL, "gatv2_logits: items/indices/fs/fd/attn/e is NULL");
    BOT_REQUIRE(ldfs >= HD && ldfd >= HD && lde >= H, BOT_E_RANGE, "gatv2_logits: row strides smaller than the rows (ldfs=%lld ldfd=%lld H*D=%d lde=%lld H=%d)",
                (long long)ldfs, (long long)ldfd, HD, (long long)lde, H);
    BOT_REQUIRE(aligned(fs, 4) && aligned(fd, 4) && aligned(attn, 4) && aligned(e, 4) && aligned(items, 16), BOT_E_ALIGN,
                "gatv2_logits: misaligned pointer");
    const Gv2Args a{indices, operm, reinterpret_cast<const int4*>(items), n_items, fs, ldfs, fd, ldfd, attn, D, HD, slope, e, lde, nullptr, 0,
                    nullptr, nullptr};
    const int vec = pick_vec(D, {ldfs, ldfd}, {fs, fd, attn});
    dispatch_sweep(Gv2Launch<GV2_FWD>{a, (hipStream_t)stream}, HD, vec);
    return hip_status("gatv2_logits launch");
}

int64_t bot_gatv2_logits_bwd_dst_workspace_floats(int64_t n_items, int64_t n_slots, int32_t H, int32_t D) {
    if (n_items < 0 || n_slots < 0 || H < 1 || D < 1) return 0;
    return (n_slots + bot::gv2_max_partials(n_items)) * (int64_t)H * D;
}

int bot_gatv2_logits_bwd_dst_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                                 const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots, const float* fs, int64_t ldfs,
                                 const float* fd, int64_t ldfd, const float* attn, int32_t H, int32_t D, float slope, const float* de, int64_t ldde,
                                 const int32_t* dperm, float* dfd, int64_t lddfd, float* dattn, float* workspace, bot_stream_t stream) {
    using namespace bot;
    (void)indptr;
    GV2_COMMON("gatv2_logits_bwd_dst")
    BOT_REQUIRE(n_long >= 0 && n_slots >= 0, BOT_E_RANGE, "gatv2_logits_bwd_dst: negative size");
    if (n_rows == 0 || (!dfd && !dattn)) return 0;
    const int32_t HD = H * D;
    BOT_REQUIRE(items && fs && fd && attn, BOT_E_NULL, "gatv2_logits_bwd_dst: items/fs/fd/attn is NULL");
    BOT_REQUIRE(nnz == 0 || (indices && de), BOT_E_NULL, "gatv2_logits_bwd_dst: indices/de is NULL");
    BOT_REQUIRE(workspace || (!dattn && n_long == 0), BOT_E_NULL, "gatv2_logits_bwd_dst: dattn and long rows need the workspace");
    BOT_REQUIRE(n_long == 0 || (long_rows && long_ptr), BOT_E_NULL, "gatv2_logits_bwd_dst: long rows need long_rows/long_ptr");
    BOT_REQUIRE(n_long == 0 || n_slots > 0, BOT_E_RANGE, "gatv2_logits_bwd_dst: long rows without slots");
    BOT_REQUIRE(ldfs >= HD && ldfd >= HD && ldde >= H && (!dfd || lddfd >= HD), BOT_E_RANGE,
                "gatv2_logits_bwd_dst: row strides smaller than the rows (ldfs=%lld ldfd=%lld lddfd=%lld H*D=%d ldde=%lld H=%d)", (long long)ldfs,
                (long long)ldfd, (long long)lddfd, HD, (long long)ldde, H);
    BOT_REQUIRE(dfd != fd && dfd != fs, BOT_E_RANGE, "gatv2_logits_bwd_dst: dfd aliases an input");
    BOT_REQUIRE(aligned(fs, 4) && aligned(fd, 4) && aligned(attn, 4) && aligned(de, 4) && aligned(dfd, 4) && aligned(dattn, 4) && aligned(items, 16) && aligned(workspace, 16),
                BOT_E_ALIGN, "gatv2_logits_bwd_dst: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    float* dpart = dattn ? workspace + n_slots * HD : nullptr;
    const Gv2Args a{indices, dperm, reinterpret_cast<const int4*>(items), n_items, fs, ldfs, fd, ldfd, attn, D, HD, slope, const_cast<float*>(de), ldde,
                    dfd, lddfd, workspace, dpart};
    const int vec = pick_vec(D, {ldfs, ldfd, dfd ? lddfd : 0}, {fs, fd, attn, dfd});  // (the workspace: 16-byte base, rows of H*D floats)
    const int64_t blocks = dispatch_sweep(Gv2Launch<GV2_BWD_DST>{a, st}, HD, vec);
    if (int rc = hip_status("gatv2_logits_bwd_dst launch")) return rc;
    if (dfd && n_long > 0) {
        launch_sum_combine(workspace, HD, dfd, lddfd, long_rows, long_ptr, n_long, st);
        if (int rc = hip_status("gatv2_logits_bwd_dst combine launch")) return rc;
    }
    if (dattn) {
        hipLaunchKernelGGL(gatv2_dattn_reduce_kernel, dim3((unsigned)(((int64_t)HD * kWave + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, dpart,
                           (int32_t)blocks, HD, dattn);
        if (int rc = hip_status("gatv2_logits_bwd_dst dattn reduce launch")) return rc;
    }
    return 0;
}

int bot_gatv2_logits_bwd_src_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                                 const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, const int32_t* pos, const float* fs, int64_t ldfs,
                                 const float* fd, int64_t ldfd, const float* attn, int32_t H, int32_t D, float slope, const float* de, int64_t ldde,
                                 float* dfs, int64_t lddfs, float* partial, bot_stream_t stream) {
    using namespace bot;
    (void)indptr;
    GV2_COMMON("gatv2_logits_bwd_src")
    BOT_REQUIRE(n_long >= 0, BOT_E_RANGE, "gatv2_logits_bwd_src: negative size");
    if (n_rows == 0) return 0;
    const int32_t HD = H * D;
    if (int rc = check_plan("gatv2_logits_bwd_src", items, "items/fs/attn/dfs", fs && attn && dfs, nnz, "indices/pos/fd/de",
                            indices && pos && fd && de, n_long, "long_rows/long_ptr/partial", long_rows && long_ptr && partial))
        return rc;
    BOT_REQUIRE(ldfs >= HD && ldfd >= HD && ldde >= H && lddfs >= HD, BOT_E_RANGE,
                "gatv2_logits_bwd_src: row strides smaller than the rows (ldfs=%lld ldfd=%lld lddfs=%lld H*D=%d ldde=%lld H=%d)", (long long)ldfs,
                (long long)ldfd, (long long)lddfs, HD, (long long)ldde, H);
    BOT_REQUIRE(dfs != fd && dfs != fs, BOT_E_RANGE, "gatv2_logits_bwd_src: dfs aliases an input");
    BOT_REQUIRE(aligned(fs, 4) && aligned(fd, 4) && aligned(attn, 4) && aligned(de, 4) && aligned(dfs, 4) && aligned(items, 16) && aligned(partial, 16),
                BOT_E_ALIGN, "gatv2_logits_bwd_src: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    const Gv2Args a{indices, pos, reinterpret_cast<const int4*>(items), n_items, fs, ldfs, fd, ldfd, attn, D, HD, slope, const_cast<float*>(de), ldde,
                    dfs, lddfs, partial, nullptr};
    const int vec = pick_vec(D, {ldfs, ldfd, lddfs}, {fs, fd, attn, dfs});
    dispatch_sweep(Gv2Launch<GV2_BWD_SRC>{a, st}, HD, vec);
    if (int rc = hip_status("gatv2_logits_bwd_src launch")) return rc;
    if (n_long > 0) {
        launch_sum_combine(partial, HD, dfs, lddfs, long_rows, long_ptr, n_long, st);
        if (int rc = hip_status("gatv2_logits_bwd_src combine launch")) return rc;
    }
    return 0;
}

}  // extern "C"
