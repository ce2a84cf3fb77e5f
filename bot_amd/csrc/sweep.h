// What the plan-driven single-head gather kernels (spmm.hip spmm_kernel, propagate.hip, spmm_max.hip, spmm_softmax.hip, gatv2.hip) share.  They are one
// lane-group row sweep (MI355X_MICROARCH.md "Indexed rows", cdna_hip_programming.md Appendix B "Scatter / gather"): one LANES-wide lane
// group (8 / 16 / 32 / 64) per work item of the row plan, lanes across the columns with 4 / 8 / 16-byte loads, so a 40-column row is 10
// lanes and one gather instruction of a wavefront fetches the rows of four items; the ids of a row are read LANES at a time, each lane
// with at most one more 32-bit word of its edge, and broadcast lane by lane, four neighbour rows in flight per group.  Here: the decode of
// a plan item (load_item), a lane's columns (ColTile), where a group's sums go (sum_row), the neighbour walk (walk_row), the slot-order
// sum of a long row's chunks (launch_sum_combine), the ladder of instances (dispatch_sweep) and the entry points' checks of the plan
// arguments (check_plan_sizes, check_plan).  Which kernels run on walk_row and which keep the walk written out, and why: DESIGN.md §4, §8.
#pragma once
#include "common.h"

namespace bot {

struct RowItem {
    int row, beg, end, slot;  // positions [beg, end) of `row`; slot >= 0: a chunk of a long row, its row of the partial workspace
};

template <int LANES>
__device__ __forceinline__ RowItem load_item(const int4* items, int64_t item) {
    const int4 it = items[item];
    RowItem r{it.x, it.y, it.z, it.w};
    if constexpr (LANES == 64) {  // wave-uniform: keep them in SGPRs
        r.row = __builtin_amdgcn_readfirstlane(r.row);
        r.beg = __builtin_amdgcn_readfirstlane(r.beg);
        r.end = __builtin_amdgcn_readfirstlane(r.end);
        r.slot = __builtin_amdgcn_readfirstlane(r.slot);
    }
    return r;
}

// The columns of one lane in a tile of LANES * VEC * NCHUNK that starts at col0: chunk c is VEC columns from off[c], act[c] where they
// are below ncols.
template <int VEC, int LANES, int NCHUNK>
struct ColTile {
    int off[NCHUNK];
    bool act[NCHUNK];
    __device__ __forceinline__ ColTile(int col0, int lane, int ncols) {
#pragma unroll
        for (int c = 0; c < NCHUNK; ++c) {
            const int e = col0 + (c * LANES + lane) * VEC;
            act[c] = e < ncols;
            off[c] = act[c] ? e : 0;  // idle lanes re-read column 0: always in bounds, never stored
        }
    }
    // the lane's sums into the row that starts at `base`
    __device__ __forceinline__ void store(float* base, const float (&acc)[NCHUNK][VEC]) const {
#pragma unroll
        for (int c = 0; c < NCHUNK; ++c)
            if (act[c]) vstore<VEC>(base + off[c], acc[c]);
    }
};

// Where a group's sums go: its row of `out`, or - a chunk of a long row - its row of `partial` ([n_slots, ncols], added by launch_sum_combine)
__device__ __forceinline__ float* sum_row(const RowItem& it, float* out, int64_t ldo, float* partial, int ncols) {
    return it.slot >= 0 ? partial + (int64_t)it.slot * ncols : out + (int64_t)it.row * ldo;
}

struct Edge {
    int id, word;  // the source row of a position and one more 32-bit word of it (a float travels as its bits)
};

// The walk over positions [beg, end) by a LANES-wide group:
//   read(k, in)           -> Edge   per lane: position k = k0 + lane, `in` where k < end (the loads of the ids' level)
//   fetch(id, word, st, k)          the group: the row loads of the neighbour of position k into the staging slot st (a Stage); k is
//                                   for operands read per POSITION beside the neighbour's rows (dot_attn.hip's edge features)
//   use(id, word, st, k)            the group: consumes the neighbour of position k
// All U fetches of a batch are issued before its first use, so U neighbour rows are in flight per group; then the scalar tail.
template <int LANES, class Stage, int U = 4, class Read, class Fetch, class Use>
__device__ __forceinline__ void walk_row(int beg, int end, int lane, Read&& read, Fetch&& fetch, Use&& use) {
    for (int k0 = beg; k0 < end; k0 += LANES) {
        const int k = k0 + lane;
        const Edge e = read(k, k < end);
        const int cnt = min(LANES, end - k0);
        int i = 0;
        for (; i + U <= cnt; i += U) {
            Stage st[U];
            int s[U], w[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                s[u] = group_bcast<LANES>(e.id, i + u);
                w[u] = group_bcast<LANES>(e.word, i + u);
                fetch(s[u], w[u], st[u], k0 + i + u);
            }
#pragma unroll
            for (int u = 0; u < U; ++u) use(s[u], w[u], st[u], k0 + i + u);
        }
        for (; i < cnt; ++i) {
            Stage st;
            const int s = group_bcast<LANES>(e.id, i);
            const int w = group_bcast<LANES>(e.word, i);
            fetch(s, w, st, k0 + i);
            use(s, w, st, k0 + i);
        }
    }
}

// out[long_rows[i], c] = partial[long_ptr[i], c] + ... + partial[long_ptr[i + 1] - 1, c] for c < ncols, in slot order, four loads in
// flight; partial is [n_slots, ncols] (spmm.hip: spmm_combine_kernel with one head)
void launch_sum_combine(const float* partial, int32_t ncols, float* out, int64_t ldo, const int32_t* long_rows, const int32_t* long_ptr,
                        int64_t n_long, hipStream_t st);

// The instance for rows of ncols columns read `vec` at a time: k.run<VEC, LANES, 1>() with the narrowest group of 8 / 16 / 32 / 64 lanes
// that holds a row, k.wide<VEC>(lanes a row needs) - the kernel's choice of NCHUNK - beyond 64.
template <int VEC, class K>
static auto dispatch_lanes(const K& k, int ncols) {
    const int L = (ncols + VEC - 1) / VEC;  // lanes one row needs
    if (L <= 8) return k.template run<VEC, 8, 1>();
    if (L <= 16) return k.template run<VEC, 16, 1>();
    if (L <= 32) return k.template run<VEC, 32, 1>();
    if (L <= 64) return k.template run<VEC, 64, 1>();
    return k.template wide<VEC>(L);
}
template <class K>
static auto dispatch_sweep(const K& k, int ncols, int vec) {
    if (vec == 4) return dispatch_lanes<4>(k, ncols);
    if (vec == 2) return dispatch_lanes<2>(k, ncols);
    return dispatch_lanes<1>(k, ncols);
}

// The sizes of a row plan's arguments (n_long / n_slots: 0 where the entry point has none)
inline int check_plan_sizes(const char* who, int64_t n_rows, int64_t nnz, int64_t n_items, int64_t n_long = 0, int64_t n_slots = 0) {
    BOT_REQUIRE(n_rows >= 0 && nnz >= 0 && n_items >= 0 && n_long >= 0 && n_slots >= 0, BOT_E_RANGE, "%s: negative size", who);
    BOT_REQUIRE(nnz < INT32_MAX && n_rows < INT32_MAX, BOT_E_RANGE, "%s: int32 index range exceeded", who);
    return 0;
}

// The pointers of a row plan's arguments.  `need` names, with items, the operands every call reads or writes and `have` says whether the
// entry point's own are there; `edge_need` / `edge_have` the same for what is read per edge (nnz > 0) and `long_need` / `long_have` for
// what the chunks of long rows (n_long > 0) go through.  (The 16-byte alignment of items stays with each entry point's other alignment
// checks, behind its stride checks.)
inline int check_plan(const char* who, const void* items, const char* need, bool have, int64_t nnz, const char* edge_need, bool edge_have,
                      int64_t n_long, const char* long_need, bool long_have) {
    BOT_REQUIRE(items && have, BOT_E_NULL, "%s: %s is NULL", who, need);
    BOT_REQUIRE(nnz == 0 || edge_have, BOT_E_NULL, "%s: %s is NULL", who, edge_need);
    BOT_REQUIRE(n_long == 0 || long_have, BOT_E_NULL, "%s: long rows need %s", who, long_need);
    return 0;
}

}  // namespace bot
