// Induced-subgraph extraction for partition / cluster mini-batches (Cluster-GCN style; DGL's g.subgraph(nodes)), gfx950.
//
// Input: the parent's CSC and `nodes`, n unique parent ids in the order they are to be numbered (local id = position).  Output:
// the CSC of the subgraph the set induces, rows = nodes in their order; row i keeps the in-edges of nodes[i] whose source is in
// the set, in the parent's CSC position order, so a subgraph edge's id is its CSC position (as in a sampled block).
//
// Membership is the persistent int32 map over the parent's nodes that to_block works in (all -1 between calls): mark writes
// map[nodes[i]] = i, count and fill gather map[indices[p]] for every position p of the selected rows, unmark puts the touched
// entries back.  The work per batch is one streaming read of the selected rows per pass plus a random 4-byte gather per scanned
// edge into the map (4 * n_nodes bytes: past one XCD's L2 at S-products, inside the Infinity Cache).
//
// Rows of at most kSubLongRow positions: one wavefront per row.  The lanes stride the row 64 positions at a time, 4 strides in
// flight; the kept lanes are a 64-bit ballot, the count pass adds its popcount, the fill pass puts a kept lane at offsets[i] +
// kept so far + popcount of the ballot below the lane.  Longer rows (the hubs of a power-law graph: tens of thousands of
// in-edges against a median of tens) would hold one wave for hundreds of dependent gathers while the rest of the grid has
// finished; they go to a second kernel in which a 1024-thread workgroup takes one row 4096 positions per step, each wave a
// contiguous 256 of them, and the 16 per-wave totals are exchanged through LDS — the same order, the same bytes.  The workgroups
// of that kernel look for their long rows themselves (rows dealt round-robin, so that hubs that sit side by side in the node
// list go to different workgroups): no list of long rows, no workspace, no host read.
//
// Integer work, plain stores, no global atomics on the structure: the output is a pure function of (graph, nodes).  The
// duplicate count is an integer sum (order-free).
//
// Tally (GraphSAINT's aggregator normalisation, bot_subgraph_tally_i32): the count pass's traversal with another per-lane action:
// the lane that holds position p of a listed row whose source is in the set does tally[p] += 1, a load-add-store on its own word.
// A position belongs to one row and a row is listed once (unique ids), so no two lanes meet on a word: no atomics, and tallying
// K node sets in a row leaves, per edge, the number of sets that induce it.  A long row needs no exchange between its waves.
#include "common.h"

namespace bot {

constexpr int kSubWaves = kBlock / kWave;
constexpr int kSubUnroll = 4;                       // 64-position strides a wave keeps in flight
constexpr int kSubLongRow = 2048;                   // longer rows are the workgroup kernel's
constexpr int kSubLongBlock = 1024;
constexpr int kSubLongWaves = kSubLongBlock / kWave;
constexpr int kSubLongTile = kSubLongBlock * kSubUnroll;
constexpr unsigned long long kSubOutOfRange = 1ull << 32;   // *n_dup: duplicates + 2^32 per id outside [0, n_nodes)

__global__ __launch_bounds__(kBlock) void subgraph_mark_kernel(const int32_t* __restrict__ nodes, int64_t n, int32_t* __restrict__ map,
                                                               int64_t n_nodes, unsigned long long* n_dup) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *n_dup = 0;        // the check kernel (next in the stream) adds to it
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int32_t v = nodes[i];
        if (v >= 0 && v < n_nodes) map[v] = (int32_t)i;         // duplicates: one of the writers stays, whichever
    }
}

// a position whose entry holds another position lost it to a duplicate: of m positions naming one node exactly m - 1 lose
__global__ __launch_bounds__(kBlock) void subgraph_check_kernel(const int32_t* __restrict__ nodes, int64_t n, const int32_t* __restrict__ map,
                                                                int64_t n_nodes, unsigned long long* n_dup) {
    int32_t dup = 0, out = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int32_t v = nodes[i];
        if (v < 0 || v >= n_nodes) ++out;
        else if (map[v] != (int32_t)i) ++dup;
    }
#pragma unroll
    for (int o = kWave / 2; o > 0; o >>= 1) {
        dup += __shfl_xor(dup, o);
        out += __shfl_xor(out, o);
    }
    if ((threadIdx.x & (kWave - 1)) == 0 && (dup | out)) atomicAdd(n_dup, (unsigned long long)dup + kSubOutOfRange * (unsigned long long)out);
}

__global__ __launch_bounds__(kBlock) void subgraph_unmark_kernel(const int32_t* __restrict__ nodes, int64_t n, int32_t* __restrict__ map,
                                                                 int64_t n_nodes) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBlock) {
        const int32_t v = nodes[i];
        if (v >= 0 && v < n_nodes) map[v] = -1;
    }
}

// the row of node v: [base, base + deg); an id outside the parent's rows is an empty row (mark reports it, nothing is read)
__device__ __forceinline__ void subgraph_row(const int32_t* __restrict__ indptr, int64_t n_rows, int32_t v, int32_t& base, int32_t& deg) {
    base = 0, deg = 0;
    if (v >= 0 && v < n_rows) {
        base = indptr[v];
        deg = indptr[v + 1] - base;
    }
}

// kSubUnroll strides of 64 positions from `lo` (this wave's first position) up to `end`: the local ids of the sources (-1: not in
// the set or past the end) and the ballot of the kept lanes of each stride; returns the number kept
__device__ __forceinline__ int32_t subgraph_gather(const int32_t* __restrict__ indices, const int32_t* __restrict__ map, int64_t lo, int64_t end,
                                                   int lane, int32_t (&l)[kSubUnroll], uint64_t (&m)[kSubUnroll]) {
    int32_t u[kSubUnroll];
#pragma unroll
    for (int t = 0; t < kSubUnroll; ++t) {
        const int64_t p = lo + t * kWave + lane;
        u[t] = p < end ? indices[p] : -1;
    }
    int32_t kept = 0;
#pragma unroll
    for (int t = 0; t < kSubUnroll; ++t) {
        l[t] = u[t] >= 0 ? map[u[t]] : -1;
        m[t] = __ballot(l[t] >= 0);
        kept += __popcll(m[t]);
    }
    return kept;
}

__device__ __forceinline__ void subgraph_store(const int32_t* __restrict__ eid, int64_t lo, int lane, const int32_t (&l)[kSubUnroll],
                                               const uint64_t (&m)[kSubUnroll], int64_t slot0, int32_t* __restrict__ local_src,
                                               int32_t* __restrict__ parent_eid) {
    const uint64_t below = (1ull << lane) - 1ull;
#pragma unroll
    for (int t = 0; t < kSubUnroll; ++t) {
        if (l[t] >= 0) {
            const int64_t slot = slot0 + __popcll(m[t] & below);
            local_src[slot] = l[t];
            parent_eid[slot] = eid[lo + t * kWave + lane];
        }
        slot0 += __popcll(m[t]);
    }
}

template <bool FILL>
__global__ __launch_bounds__(kBlock) void subgraph_rows_kernel(const int32_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                               const int32_t* __restrict__ eid, int64_t n_rows, const int32_t* __restrict__ nodes,
                                                               int64_t n, const int32_t* __restrict__ map, int32_t* __restrict__ counts,
                                                               const int64_t* __restrict__ offsets, int32_t* __restrict__ local_src,
                                                               int32_t* __restrict__ parent_eid) {
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int64_t n_waves = (int64_t)gridDim.x * kSubWaves;
    for (int64_t i = (int64_t)blockIdx.x * kSubWaves + wv; i < n; i += n_waves) {
        int32_t base, deg;
        subgraph_row(indptr, n_rows, nodes[i], base, deg);
        if (deg > kSubLongRow) continue;               // subgraph_long_rows_kernel's
        const int64_t end = (int64_t)base + deg;
        int64_t slot = FILL ? offsets[i] : 0;
        int32_t kept = 0;
        for (int64_t lo = base; lo < end; lo += kSubUnroll * kWave) {
            int32_t l[kSubUnroll];
            uint64_t m[kSubUnroll];
            const int32_t c = subgraph_gather(indices, map, lo, end, lane, l, m);
            if constexpr (FILL) subgraph_store(eid, lo, lane, l, m, slot + kept, local_src, parent_eid);
            kept += c;
        }
        if (!FILL && lane == 0) counts[i] = kept;
    }
}

template <bool FILL>
__global__ __launch_bounds__(kSubLongBlock) void subgraph_long_rows_kernel(const int32_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                                           const int32_t* __restrict__ eid, int64_t n_rows,
                                                                           const int32_t* __restrict__ nodes, int64_t n, const int32_t* __restrict__ map,
                                                                           int32_t* __restrict__ counts, const int64_t* __restrict__ offsets,
                                                                           int32_t* __restrict__ local_src, int32_t* __restrict__ parent_eid) {
    __shared__ int64_t list[kSubLongBlock];           // the long rows among the 1024 this workgroup looked at in one sweep
    __shared__ int32_t n_list;
    __shared__ int32_t wsum[2][kSubLongWaves];
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int64_t sweep = (int64_t)gridDim.x * kSubLongBlock;
    for (int64_t i0 = 0; i0 < n; i0 += sweep) {
        if (threadIdx.x == 0) n_list = 0;
        __syncthreads();
        const int64_t mine = i0 + (int64_t)threadIdx.x * gridDim.x + blockIdx.x;     // neighbouring rows: different workgroups
        if (mine < n) {
            int32_t base, deg;
            subgraph_row(indptr, n_rows, nodes[mine], base, deg);
            if (deg > kSubLongRow) list[atomicAdd(&n_list, 1)] = mine;               // LDS; the order of the list changes no output
        }
        __syncthreads();
        const int32_t nl = n_list;
        for (int32_t q = 0; q < nl; ++q) {
            const int64_t i = list[q];
            int32_t base, deg;
            subgraph_row(indptr, n_rows, nodes[i], base, deg);
            const int64_t end = (int64_t)base + deg;
            const int64_t o = FILL ? offsets[i] : 0;
            int32_t kept = 0, flip = 0;                 // kept: the same in every thread
            for (int64_t t0 = base; t0 < end; t0 += kSubLongTile, flip ^= 1) {
                const int64_t lo = t0 + wv * (kSubUnroll * kWave);
                int32_t l[kSubUnroll];
                uint64_t m[kSubUnroll];
                const int32_t c = subgraph_gather(indices, map, lo, end, lane, l, m);
                if (lane == 0) wsum[flip][wv] = c;
                __syncthreads();                        // one barrier per tile: the next tile writes the other half of wsum
                int32_t before = 0, all = 0;
#pragma unroll
                for (int w = 0; w < kSubLongWaves; ++w) {
                    const int32_t s = wsum[flip][w];
                    before += w < wv ? s : 0;
                    all += s;
                }
                if constexpr (FILL) subgraph_store(eid, lo, lane, l, m, o + kept + before, local_src, parent_eid);
                kept += all;
            }
            if (!FILL && threadIdx.x == 0) counts[i] = kept;
            __syncthreads();                            // wsum[0] is written again by the next row's first tile
        }
        __syncthreads();                                // n_list / list are reused by the next sweep
    }
}

// positions [lo, lo + kSubUnroll * kWave) of one row: +1 on the kept lanes' own words
__device__ __forceinline__ void subgraph_tally_strides(const int32_t* __restrict__ indices, const int32_t* __restrict__ map, int64_t lo, int64_t end,
                                                       int lane, int32_t* __restrict__ tally) {
    int32_t l[kSubUnroll];
    uint64_t m[kSubUnroll];
    subgraph_gather(indices, map, lo, end, lane, l, m);
    int32_t c[kSubUnroll];
#pragma unroll
    for (int t = 0; t < kSubUnroll; ++t) c[t] = l[t] >= 0 ? tally[lo + t * kWave + lane] : 0;      // l >= 0 only below `end`
#pragma unroll
    for (int t = 0; t < kSubUnroll; ++t)
        if (l[t] >= 0) tally[lo + t * kWave + lane] = c[t] + 1;
}

__global__ __launch_bounds__(kBlock) void subgraph_tally_rows_kernel(const int32_t* __restrict__ indptr, const int32_t* __restrict__ indices,
                                                                     int64_t n_rows, const int32_t* __restrict__ nodes, int64_t n,
                                                                     const int32_t* __restrict__ map, int32_t* __restrict__ tally) {
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int64_t n_waves = (int64_t)gridDim.x * kSubWaves;
    for (int64_t i = (int64_t)blockIdx.x * kSubWaves + wv; i < n; i += n_waves) {
        int32_t base, deg;
        subgraph_row(indptr, n_rows, nodes[i], base, deg);
        if (deg > kSubLongRow) continue;               // subgraph_tally_long_rows_kernel's
        const int64_t end = (int64_t)base + deg;
        for (int64_t lo = base; lo < end; lo += kSubUnroll * kWave) subgraph_tally_strides(indices, map, lo, end, lane, tally);
    }
}

// the long rows, found as subgraph_long_rows_kernel finds them; each wave takes its 256 positions of a 4096-position tile
__global__ __launch_bounds__(kSubLongBlock) void subgraph_tally_long_rows_kernel(const int32_t* __restrict__ indptr,
                                                                                 const int32_t* __restrict__ indices, int64_t n_rows,
                                                                                 const int32_t* __restrict__ nodes, int64_t n,
                                                                                 const int32_t* __restrict__ map, int32_t* __restrict__ tally) {
    __shared__ int64_t list[kSubLongBlock];
    __shared__ int32_t n_list;
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int64_t sweep = (int64_t)gridDim.x * kSubLongBlock;
    for (int64_t i0 = 0; i0 < n; i0 += sweep) {
        if (threadIdx.x == 0) n_list = 0;
        __syncthreads();
        const int64_t mine = i0 + (int64_t)threadIdx.x * gridDim.x + blockIdx.x;
        if (mine < n) {
            int32_t base, deg;
            subgraph_row(indptr, n_rows, nodes[mine], base, deg);
            if (deg > kSubLongRow) list[atomicAdd(&n_list, 1)] = mine;               // LDS; the order of the list changes no output
        }
        __syncthreads();
        const int32_t nl = n_list;
        for (int32_t q = 0; q < nl; ++q) {
            int32_t base, deg;
            subgraph_row(indptr, n_rows, nodes[list[q]], base, deg);
            const int64_t end = (int64_t)base + deg;
            for (int64_t t0 = (int64_t)base + wv * (kSubUnroll * kWave); t0 < end; t0 += kSubLongTile)
                subgraph_tally_strides(indices, map, t0, end, lane, tally);
        }
        __syncthreads();                                // n_list / list are reused by the next sweep
    }
}

template <bool FILL>
inline void subgraph_launch(const int32_t* indptr, const int32_t* indices, const int32_t* eid, int64_t n_rows, const int32_t* nodes, int64_t n,
                            const int32_t* map, int32_t* counts, const int64_t* offsets, int32_t* local_src, int32_t* parent_eid, hipStream_t st) {
    // the hubs first: one workgroup per CU at most (16 rows per workgroup on a small set, so that a few hubs still spread)
    hipLaunchKernelGGL(subgraph_long_rows_kernel<FILL>, dim3(launch_grid(n, 16, 256)), dim3(kSubLongBlock), 0, st, indptr, indices, eid, n_rows,
                       nodes, n, map, counts, offsets, local_src, parent_eid);
    hipLaunchKernelGGL(subgraph_rows_kernel<FILL>, dim3(launch_grid(n, kSubWaves, 8192)), dim3(kBlock), 0, st, indptr, indices, eid, n_rows, nodes,
                       n, map, counts, offsets, local_src, parent_eid);
}

}  // namespace bot

extern "C" {

int bot_subgraph_mark_i32(const int32_t* nodes, int64_t n, int32_t* map, int64_t n_nodes, int64_t* n_dup, bot_stream_t stream) {
    using namespace bot;
    BOT_REQUIRE(n >= 0 && n_nodes >= 0 && n <= n_nodes, BOT_E_RANGE, "subgraph_mark: n=%lld n_nodes=%lld", (long long)n, (long long)n_nodes);
    BOT_REQUIRE(map != nullptr && n_dup != nullptr, BOT_E_NULL, "subgraph_mark: NULL map / n_dup");
    if (n == 0) return 0;
    BOT_REQUIRE(nodes != nullptr, BOT_E_NULL, "subgraph_mark: nodes is NULL");
    hipStream_t st = (hipStream_t)stream;
    set_kernel("subgraph_mark_kernel");
    hipLaunchKernelGGL(subgraph_mark_kernel, dim3(launch_grid(n, kBlock, 4096)), dim3(kBlock), 0, st, nodes, n, map, n_nodes,
                       (unsigned long long*)n_dup);
    hipLaunchKernelGGL(subgraph_check_kernel, dim3(launch_grid(n, kBlock, 4096)), dim3(kBlock), 0, st, nodes, n, map, n_nodes,
                       (unsigned long long*)n_dup);
    return hip_status("subgraph_mark launch");
}

int bot_subgraph_count_i32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, const int32_t* nodes, int64_t n, const int32_t* map,
                           int32_t* counts, bot_stream_t stream) {
    using namespace bot;
    BOT_REQUIRE(n_rows >= 0 && n >= 0 && n <= n_rows, BOT_E_RANGE, "subgraph_count: n_rows=%lld n=%lld", (long long)n_rows, (long long)n);
    BOT_REQUIRE(indptr != nullptr && map != nullptr, BOT_E_NULL, "subgraph_count: NULL indptr / map");
    if (n == 0) return 0;
    BOT_REQUIRE(indices != nullptr && nodes != nullptr && counts != nullptr, BOT_E_NULL, "subgraph_count: NULL indices / nodes / counts");
    set_kernel("subgraph_rows_kernel<count>");
    subgraph_launch<false>(indptr, indices, nullptr, n_rows, nodes, n, map, counts, nullptr, nullptr, nullptr, (hipStream_t)stream);
    return hip_status("subgraph_count launch");
}

int bot_subgraph_fill_i32(const int32_t* indptr, const int32_t* indices, const int32_t* eid, int64_t n_rows, const int32_t* nodes, int64_t n,
                          const int32_t* map, const int64_t* offsets, int32_t* local_src, int32_t* parent_eid, bot_stream_t stream) {
    using namespace bot;
    BOT_REQUIRE(n_rows >= 0 && n >= 0 && n <= n_rows, BOT_E_RANGE, "subgraph_fill: n_rows=%lld n=%lld", (long long)n_rows, (long long)n);
    BOT_REQUIRE(indptr != nullptr && map != nullptr, BOT_E_NULL, "subgraph_fill: NULL indptr / map");
    if (n == 0) return 0;
    BOT_REQUIRE(indices != nullptr && eid != nullptr && nodes != nullptr && offsets != nullptr && local_src != nullptr && parent_eid != nullptr,
                BOT_E_NULL, "subgraph_fill: NULL indices / eid / nodes / offsets / local_src / parent_eid");
    set_kernel("subgraph_rows_kernel<fill>");
    subgraph_launch<true>(indptr, indices, eid, n_rows, nodes, n, map, nullptr, offsets, local_src, parent_eid, (hipStream_t)stream);
    return hip_status("subgraph_fill launch");
}

int bot_subgraph_tally_i32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, const int32_t* nodes, int64_t n, const int32_t* map,
                           int32_t* tally, bot_stream_t stream) {
    using namespace bot;
    BOT_REQUIRE(n_rows >= 0 && n >= 0 && n <= n_rows, BOT_E_RANGE, "subgraph_tally: n_rows=%lld n=%lld", (long long)n_rows, (long long)n);
    BOT_REQUIRE(indptr != nullptr && map != nullptr, BOT_E_NULL, "subgraph_tally: NULL indptr / map");
    if (n == 0) return 0;
    BOT_REQUIRE(indices != nullptr && nodes != nullptr && tally != nullptr, BOT_E_NULL, "subgraph_tally: NULL indices / nodes / tally");
    hipStream_t st = (hipStream_t)stream;
    set_kernel("subgraph_tally_rows_kernel");
    hipLaunchKernelGGL(subgraph_tally_long_rows_kernel, dim3(launch_grid(n, 16, 256)), dim3(kSubLongBlock), 0, st, indptr, indices, n_rows, nodes, n,
                       map, tally);
    hipLaunchKernelGGL(subgraph_tally_rows_kernel, dim3(launch_grid(n, kSubWaves, 8192)), dim3(kBlock), 0, st, indptr, indices, n_rows, nodes, n, map,
                       tally);
    return hip_status("subgraph_tally launch");
}

int bot_subgraph_unmark_i32(const int32_t* nodes, int64_t n, int32_t* map, int64_t n_nodes, bot_stream_t stream) {
    using namespace bot;
    BOT_REQUIRE(n >= 0 && n_nodes >= 0 && n <= n_nodes, BOT_E_RANGE, "subgraph_unmark: n=%lld n_nodes=%lld", (long long)n, (long long)n_nodes);
    BOT_REQUIRE(map != nullptr, BOT_E_NULL, "subgraph_unmark: map is NULL");
    if (n == 0) return 0;
    BOT_REQUIRE(nodes != nullptr, BOT_E_NULL, "subgraph_unmark: nodes is NULL");
    set_kernel("subgraph_unmark_kernel");
    hipLaunchKernelGGL(subgraph_unmark_kernel, dim3(launch_grid(n, kBlock, 4096)), dim3(kBlock), 0, (hipStream_t)stream, nodes, n, map, n_nodes);
    return hip_status("subgraph_unmark launch");
}

}  // extern "C"
