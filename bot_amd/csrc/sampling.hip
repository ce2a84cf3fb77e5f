// Neighbour sampling without replacement and block construction (DGL's MultiLayerNeighborSampler + to_block, as the reference's
// ogbn-products / ogbn-proteins scripts use them: src/ogbn-products/gat.py:196-235, src/ogbn-proteins/gat.py:174-200), gfx950.
//
// Sampling.  For seed v with in-degree deg (CSC row of the parent graph) and fan-out k, c = min(deg, k) in-edges are picked
// uniformly without replacement (k < 0: all of them).  Rows with deg <= k are copied whole by the lanes of one wavefront.  Longer
// rows run Floyd's algorithm: for j = deg - k .. deg - 1, t = uniform{0..j}; take t unless it was taken already, then take j.
// The draw for step j of row v is umulhi64(r, j + 1) with r the first 64 bits of Philox4x32-10(seed, counter = v << 32 | j):
// bias below 2^-32 for any row length, and a pure function of (v, j, seed) — independent of where v sits in the seed list,
// of the launch shape and of the run.  A wavefront does one row: the 64 lanes draw 64 steps ahead, test membership of the
// taken set (LDS) in parallel, and finally write the k positions in ascending order (rank of each among the taken set).
// O(k^2 / 64) per row, never O(deg): a hub of 10^5 in-edges costs what a row of k + 1 does.
//
// Block construction.  The block's sources are the seeds (in their given order), then every newly reached parent node once in
// ascending parent id.  A persistent int32 map over the parent's nodes holds -1 between calls: the seeds are marked with their
// positions, reached nodes with -2; a tiled exclusive scan over the map assigns the new ids in ascending id; the sampled edges
// are relabelled through the map; finally only the touched entries are reset to -1.  Plain stores and integer arithmetic only
// (concurrent writers of one entry store the same value): deterministic.
#include "common.h"

namespace bot {

constexpr int kSampleMaxK = 1024;               // largest fan-out of the without-replacement path (the reference uses 8..100)
constexpr int kSampleWaves = kBlock / kWave;
constexpr int kMapTile = kBlock * 8;            // map entries per workgroup of the scan

__device__ __forceinline__ uint32_t floyd_draw(uint64_t seed, int32_t v, int32_t j) {
    return (uint32_t)__umul64hi(Philox::word64(seed, (uint32_t)v, (uint32_t)j), (uint64_t)(uint32_t)j + 1u);
}

__global__ __launch_bounds__(kBlock) void sample_count_kernel(const int32_t* indptr, const int32_t* seeds, int64_t n_seeds, int32_t k,
                                                              int32_t* counts) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_seeds; i += (int64_t)gridDim.x * kBlock) {
        const int32_t v = seeds[i];
        const int32_t deg = indptr[v + 1] - indptr[v];
        counts[i] = (k < 0 || deg <= k) ? deg : k;
    }
}

__global__ __launch_bounds__(kBlock) void sample_rows_kernel(const int32_t* indptr, const int32_t* seeds, int64_t n_seeds, int32_t k,
                                                             uint64_t seed, const int64_t* offsets, int32_t* out) {
    __shared__ int32_t taken_all[kSampleWaves][kSampleMaxK];
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    int32_t* taken = taken_all[wv];
    const int64_t n_waves = (int64_t)gridDim.x * kSampleWaves;
    for (int64_t i = (int64_t)blockIdx.x * kSampleWaves + wv; i < n_seeds; i += n_waves) {
        const int32_t v = seeds[i];
        const int32_t base = indptr[v], deg = indptr[v + 1] - base;
        const int64_t o = offsets[i];
        if (k < 0 || deg <= k) {                       // the whole row, in position order
            for (int32_t j = lane; j < deg; j += kWave) out[o + j] = base + j;
            continue;
        }
        const int32_t first = deg - k;
        for (int32_t m0 = 0; m0 < k; m0 += kWave) {
            const uint32_t mine = (m0 + lane < k) ? floyd_draw(seed, v, first + m0 + lane) : 0u;
            const int32_t steps = min(kWave, k - m0);
            for (int32_t s = 0; s < steps; ++s) {
                const int32_t m = m0 + s;
                const int32_t t = (int32_t)__shfl(mine, s);
                bool hit = false;
                for (int32_t q = lane; q < m; q += kWave) hit |= taken[q] == t;
                const int32_t pick = __any(hit) ? first + m : t;
                if (lane == 0) taken[m] = pick;
                lds_wave_fence();                      // the LDS store lands before any lane reads it back
            }
        }
        for (int32_t q = lane; q < k; q += kWave) {   // ascending order: each taken offset goes to its rank
            const int32_t x = taken[q];
            int32_t rank = 0;
            for (int32_t r = 0; r < k; ++r) rank += taken[r] < x;
            out[o + rank] = base + x;
        }
        __builtin_amdgcn_wave_barrier();               // the next row overwrites `taken`
    }
}

__global__ __launch_bounds__(kBlock) void block_seed_kernel(const int32_t* seeds, int64_t n_seeds, int32_t* map) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_seeds; i += (int64_t)gridDim.x * kBlock) map[seeds[i]] = (int32_t)i;
}

__global__ __launch_bounds__(kBlock) void block_reach_kernel(const int32_t* indices, const int32_t* pos, int64_t n_pos, int32_t* map) {
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n_pos; e += (int64_t)gridDim.x * kBlock) {
        const int32_t u = indices[pos[e]];
        if (map[u] == -1) map[u] = -2;              // every writer stores the same value
    }
}

// exclusive scan of one value per thread over the workgroup; returns the workgroup total in *total
__device__ __forceinline__ int32_t block_exclusive_scan(int32_t x, int32_t* total) {
    __shared__ int32_t wsum[kSampleWaves];
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int32_t inc = wave_inclusive_scan(x, lane);
    if (lane == kWave - 1) wsum[wv] = inc;
    __syncthreads();
    int32_t before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < kSampleWaves; ++w) {
        before += w < wv ? wsum[w] : 0;
        all += wsum[w];
    }
    __syncthreads();
    *total = all;
    return before + inc - x;
}

__global__ __launch_bounds__(kBlock) void block_tile_count_kernel(const int32_t* map, int64_t n_nodes, int64_t* tile_counts) {
    const int64_t lo = (int64_t)blockIdx.x * kMapTile + threadIdx.x * 8;
    int32_t c = 0;
#pragma unroll
    for (int t = 0; t < 8; ++t) c += (lo + t < n_nodes && map[lo + t] == -2);
    int32_t total;
    block_exclusive_scan(c, &total);
    if (threadIdx.x == 0) tile_counts[blockIdx.x] = total;
}

// one workgroup: tile_counts -> exclusive tile offsets, the grand total into *n_new
__global__ __launch_bounds__(kBlock) void block_tile_scan_kernel(int64_t* tile_counts, int64_t n_tiles, int64_t* n_new) {
    __shared__ int64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (int64_t a = 0; a < n_tiles; a += kBlock) {
        const int64_t t = a + threadIdx.x;
        const int32_t c = t < n_tiles ? (int32_t)tile_counts[t] : 0;   // at most kMapTile per tile
        int32_t total;
        const int32_t ex = block_exclusive_scan(c, &total);
        if (t < n_tiles) tile_counts[t] = carry + ex;
        __syncthreads();
        if (threadIdx.x == 0) carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) *n_new = carry;
}

__global__ __launch_bounds__(kBlock) void block_assign_kernel(int32_t* map, int64_t n_nodes, const int64_t* tile_offsets, int64_t n_seeds,
                                                              int32_t* src_nid) {
    const int64_t lo = (int64_t)blockIdx.x * kMapTile + threadIdx.x * 8;
    int32_t f[8], c = 0;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        f[t] = lo + t < n_nodes && map[lo + t] == -2;
        c += f[t];
    }
    int32_t total;
    int64_t id = n_seeds + tile_offsets[blockIdx.x] + block_exclusive_scan(c, &total);
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        if (!f[t]) continue;
        map[lo + t] = (int32_t)id;
        src_nid[id] = (int32_t)(lo + t);
        ++id;
    }
}

__global__ __launch_bounds__(kBlock) void block_relabel_kernel(const int32_t* seeds, int64_t n_seeds, const int32_t* indices,
                                                               const int32_t* eid, const int32_t* pos, int64_t n_pos, const int32_t* map,
                                                               int32_t* src_nid, int32_t* local, int32_t* parent_eid) {
    const int64_t n = n_pos > n_seeds ? n_pos : n_seeds;
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < n; e += (int64_t)gridDim.x * kBlock) {
        if (e < n_seeds) src_nid[e] = seeds[e];
        if (e < n_pos) {
            const int32_t p = pos[e];
            local[e] = map[indices[p]];
            parent_eid[e] = eid[p];
        }
    }
}

__global__ __launch_bounds__(kBlock) void block_reset_kernel(const int32_t* src_nid, int64_t n_src, int32_t* map) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_src; i += (int64_t)gridDim.x * kBlock) map[src_nid[i]] = -1;
}

// GraphSAINT's node list (the walks are saint.hip's): every entry of `trace` marks its node as reached; the scan and the assign kernel above
// then list the marked nodes in ascending id.  An id outside [0, n_nodes) is skipped and counted.
__global__ __launch_bounds__(kBlock) void saint_mark_kernel(const int32_t* trace, int64_t n_trace, int32_t* map, int64_t n_nodes,
                                                            unsigned long long* n_bad) {
    int32_t bad = 0;
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_trace; i += (int64_t)gridDim.x * kBlock) {
        const int32_t v = trace[i];
        if (v >= 0 && v < n_nodes) map[v] = -2;     // every writer stores the same value
        else ++bad;
    }
    if (bad) atomicAdd(n_bad, (unsigned long long)bad);   // a report, never taken on a valid trace; an integer sum (order-free)
}

}  // namespace bot

extern "C" {

int bot_sample_neighbors_count_i32(const int32_t* indptr, int64_t n_rows, const int32_t* seeds, int64_t n_seeds, int32_t k, int32_t* counts,
                                   bot_stream_t stream) {
    using namespace bot;
    BOT_REQUIRE(n_rows >= 0 && n_seeds >= 0 && k <= kSampleMaxK, BOT_E_RANGE, "sample_neighbors_count: n_rows=%lld n_seeds=%lld k=%d (k <= %d)",
                (long long)n_rows, (long long)n_seeds, (int)k, kSampleMaxK);
    BOT_REQUIRE(indptr != nullptr, BOT_E_NULL, "sample_neighbors_count: indptr is NULL");
    if (n_seeds == 0) return 0;
    BOT_REQUIRE(seeds != nullptr && counts != nullptr, BOT_E_NULL, "sample_neighbors_count: NULL seeds / counts");
    set_kernel("sample_count_kernel");
    hipLaunchKernelGGL(sample_count_kernel, dim3(launch_grid(n_seeds, kBlock)), dim3(kBlock), 0, (hipStream_t)stream, indptr, seeds, n_seeds, k, counts);
    return hip_status("sample_neighbors_count launch");
}

int bot_sample_neighbors_i32(const int32_t* indptr, int64_t n_rows, const int32_t* seeds, int64_t n_seeds, int32_t k, uint64_t seed,
                             const int64_t* offsets, int32_t* out, bot_stream_t stream) {
    using namespace bot;
    BOT_REQUIRE(n_rows >= 0 && n_seeds >= 0 && k <= kSampleMaxK, BOT_E_RANGE, "sample_neighbors: n_rows=%lld n_seeds=%lld k=%d (k <= %d)",
                (long long)n_rows, (long long)n_seeds, (int)k, kSampleMaxK);
    BOT_REQUIRE(indptr != nullptr, BOT_E_NULL, "sample_neighbors: indptr is NULL");
    if (n_seeds == 0) return 0;
    BOT_REQUIRE(seeds != nullptr && offsets != nullptr && out != nullptr, BOT_E_NULL, "sample_neighbors: NULL seeds / offsets / out");
    set_kernel("sample_rows_kernel");
    hipLaunchKernelGGL(sample_rows_kernel, dim3(launch_grid(n_seeds, kSampleWaves, 8192)), dim3(kBlock), 0, (hipStream_t)stream, indptr, seeds,
                       n_seeds, k, seed, offsets, out);
    return hip_status("sample_neighbors launch");
}

int64_t bot_block_tiles(int64_t n_nodes) { return n_nodes < 0 ? 0 : (n_nodes + bot::kMapTile - 1) / bot::kMapTile; }

int bot_block_mark_i32(const int32_t* seeds, int64_t n_seeds, const int32_t* indices, const int32_t* pos, int64_t n_pos, int32_t* map,
                       int64_t n_nodes, int64_t* tile_counts, int64_t* n_new, bot_stream_t stream) {
    using namespace bot;
    BOT_REQUIRE(n_seeds >= 0 && n_pos >= 0 && n_nodes >= 0 && n_seeds <= n_nodes, BOT_E_RANGE, "block_mark: n_seeds=%lld n_pos=%lld n_nodes=%lld",
                (long long)n_seeds, (long long)n_pos, (long long)n_nodes);
    BOT_REQUIRE(map != nullptr && n_new != nullptr, BOT_E_NULL, "block_mark: NULL map / n_new");
    if (n_seeds == 0) return 0;
    BOT_REQUIRE(seeds != nullptr && tile_counts != nullptr && (n_pos == 0 || (indices != nullptr && pos != nullptr)), BOT_E_NULL,
                "block_mark: NULL seeds / tile_counts / indices / pos");
    hipStream_t st = (hipStream_t)stream;
    const int64_t n_tiles = bot_block_tiles(n_nodes);
    set_kernel("block_tile_scan_kernel");
    hipLaunchKernelGGL(block_seed_kernel, dim3(launch_grid(n_seeds, kBlock)), dim3(kBlock), 0, st, seeds, n_seeds, map);
    if (n_pos) hipLaunchKernelGGL(block_reach_kernel, dim3(launch_grid(n_pos, kBlock)), dim3(kBlock), 0, st, indices, pos, n_pos, map);
    hipLaunchKernelGGL(block_tile_count_kernel, dim3((unsigned)n_tiles), dim3(kBlock), 0, st, map, n_nodes, tile_counts);
    hipLaunchKernelGGL(block_tile_scan_kernel, dim3(1), dim3(kBlock), 0, st, tile_counts, n_tiles, n_new);
    return hip_status("block_mark launch");
}

int bot_block_relabel_i32(const int32_t* seeds, int64_t n_seeds, const int32_t* indices, const int32_t* eid, const int32_t* pos, int64_t n_pos,
                          int32_t* map, int64_t n_nodes, const int64_t* tile_offsets, int64_t n_src, int32_t* src_nid, int32_t* local,
                          int32_t* parent_eid, bot_stream_t stream) {
    using namespace bot;
    BOT_REQUIRE(n_seeds >= 0 && n_pos >= 0 && n_nodes >= 0 && n_seeds <= n_src && n_src <= n_nodes, BOT_E_RANGE,
                "block_relabel: n_seeds=%lld n_pos=%lld n_src=%lld n_nodes=%lld", (long long)n_seeds, (long long)n_pos, (long long)n_src,
                (long long)n_nodes);
    BOT_REQUIRE(map != nullptr, BOT_E_NULL, "block_relabel: map is NULL");
    if (n_seeds == 0) return 0;
    BOT_REQUIRE(seeds != nullptr && tile_offsets != nullptr && src_nid != nullptr, BOT_E_NULL, "block_relabel: NULL seeds / tile_offsets / src_nid");
    BOT_REQUIRE(n_pos == 0 || (indices != nullptr && eid != nullptr && pos != nullptr && local != nullptr && parent_eid != nullptr), BOT_E_NULL,
                "block_relabel: NULL edge arrays");
    hipStream_t st = (hipStream_t)stream;
    set_kernel("block_relabel_kernel");
    hipLaunchKernelGGL(block_assign_kernel, dim3((unsigned)bot_block_tiles(n_nodes)), dim3(kBlock), 0, st, map, n_nodes, tile_offsets, n_seeds,
                       src_nid);
    const int64_t n = n_pos > n_seeds ? n_pos : n_seeds;
    hipLaunchKernelGGL(block_relabel_kernel, dim3(launch_grid(n, kBlock)), dim3(kBlock), 0, st, seeds, n_seeds, indices, eid, pos, n_pos, map,
                       src_nid, local, parent_eid);
    hipLaunchKernelGGL(block_reset_kernel, dim3(launch_grid(n_src, kBlock)), dim3(kBlock), 0, st, src_nid, n_src, map);
    return hip_status("block_relabel launch");
}

int bot_saint_nodes_mark_i32(const int32_t* trace, int64_t n_trace, int32_t* map, int64_t n_nodes, int64_t* tile_counts, int64_t* n_out,
                             bot_stream_t stream) {
    using namespace bot;
    BOT_REQUIRE(n_trace >= 0 && n_nodes >= 0, BOT_E_RANGE, "saint_nodes_mark: n_trace=%lld n_nodes=%lld", (long long)n_trace, (long long)n_nodes);
    BOT_REQUIRE(map != nullptr && n_out != nullptr, BOT_E_NULL, "saint_nodes_mark: NULL map / n_out");
    if (n_trace == 0) return 0;
    BOT_REQUIRE(trace != nullptr && tile_counts != nullptr, BOT_E_NULL, "saint_nodes_mark: NULL trace / tile_counts");
    hipStream_t st = (hipStream_t)stream;
    const int64_t n_tiles = bot_block_tiles(n_nodes);
    set_kernel("saint_mark_kernel");
    hipLaunchKernelGGL(saint_mark_kernel, dim3(launch_grid(n_trace, kBlock)), dim3(kBlock), 0, st, trace, n_trace, map, n_nodes,
                       (unsigned long long*)(n_out + 1));
    if (n_tiles) hipLaunchKernelGGL(block_tile_count_kernel, dim3((unsigned)n_tiles), dim3(kBlock), 0, st, map, n_nodes, tile_counts);
    hipLaunchKernelGGL(block_tile_scan_kernel, dim3(1), dim3(kBlock), 0, st, tile_counts, n_tiles, n_out);
    return hip_status("saint_nodes_mark launch");
}

int bot_saint_nodes_list_i32(int32_t* map, int64_t n_nodes, const int64_t* tile_offsets, int64_t n, int32_t* nodes, bot_stream_t stream) {
    using namespace bot;
    BOT_REQUIRE(n >= 0 && n_nodes >= 0 && n <= n_nodes, BOT_E_RANGE, "saint_nodes_list: n=%lld n_nodes=%lld", (long long)n, (long long)n_nodes);
    BOT_REQUIRE(map != nullptr, BOT_E_NULL, "saint_nodes_list: map is NULL");
    if (n == 0) return 0;
    BOT_REQUIRE(tile_offsets != nullptr && nodes != nullptr, BOT_E_NULL, "saint_nodes_list: NULL tile_offsets / nodes");
    hipStream_t st = (hipStream_t)stream;
    set_kernel("block_assign_kernel");
    hipLaunchKernelGGL(block_assign_kernel, dim3((unsigned)bot_block_tiles(n_nodes)), dim3(kBlock), 0, st, map, n_nodes, tile_offsets, (int64_t)0, nodes);
    hipLaunchKernelGGL(block_reset_kernel, dim3(launch_grid(n, kBlock)), dim3(kBlock), 0, st, nodes, n, map);
    return hip_status("saint_nodes_list launch");
}

}  // extern "C"
