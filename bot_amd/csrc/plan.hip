// The graph builder of a mini-batch on the device, gfx950: the row plan of a compressed direction and the transpose of a finished CSC.
// include/bot_gnn.h "Row plan": bot_row_plan_size_device / bot_row_plan_fill_device, bot_csc_transpose_i32.
//
// Every array is held bit for bit to the host code (bot_row_plan_*_host; graph.build_direction).  Integer arithmetic only; the only
// atomics are the LDS histograms of radix.h and the count of bad indices, and none of them decides a position, so every output is a pure
// function of the input for every launch shape.  No kernel waits for another workgroup: the scans are launches of their own.
//
// Row plan.  key(r) = chunk - deg(r) for a whole row (deg <= chunk), chunk + 1 for a long one: a stable sort of the rows by key is the
// host planner's counting sort (degree descending, stable in the row id) with the long rows behind it.
//   size group   plan_tile_kernel        per tile of 2048 rows: keys, and the tile's long rows / pieces / rows with a negative degree
//                plan_tile_scan_kernel   exclusive prefix over the tiles; the three totals into `sizes`
//                1 or 2 radix passes     rows by key (radix.h)
//   fill group   plan_fill_whole_kernel  item n_slots + i = the i-th sorted row
//                plan_fill_long_kernel   long_rows / long_ptr: the in-tile rank of each long row on top of the tile's prefix
//                plan_fill_slots_kernel  one lane per PIECE (not per row: a hub row is cut by as many lanes as it has pieces), its long row
//                                        found by binary search in long_ptr
//
// Transpose.  A stable sort of the CSC positions by their source id: inside a source row the entries ascend in CSC position, which is
// argsort(stable=True)'s order.  transpose_prep_kernel (keys, positions, range check), 1 to 4 radix passes (8 bits of the source id
// each), transpose_finish_kernel: the destination row of each entry by binary search in indptr, indptr_r by binary search in the sorted keys.
#include "common.h"
#include "radix.h"

namespace bot {

constexpr int kPlanRows = 8, kPlanTile = kBlock * kPlanRows;      // 2048 rows per tile
constexpr int32_t kPlanMaxChunk = 1024;

static inline int64_t plan_align(int64_t x) { return (x + 255) / 256 * 256; }

struct PlanWorkspace {
    int64_t keys_a, keys_b, rows_a, rows_b, hist, tile, total;     // byte offsets
    int64_t tiles;
};

static PlanWorkspace plan_workspace(int64_t n_rows) {
    PlanWorkspace w;
    w.tiles = (n_rows + kPlanTile - 1) / kPlanTile;
    int64_t o = 0;
    w.keys_a = o, o += plan_align(n_rows * 4);
    w.keys_b = o, o += plan_align(n_rows * 4);
    w.rows_a = o, o += plan_align(n_rows * 4);
    w.rows_b = o, o += plan_align(n_rows * 4);
    w.hist = o, o += plan_align(radix_tiles(n_rows) * 256 * 4);
    w.tile = o, o += plan_align(w.tiles * 3 * 8);
    w.total = o;
    return w;
}

static inline int plan_passes(int32_t chunk) { return chunk + 1 < 256 ? 1 : 2; }      // keys 0 .. chunk + 1

__device__ __forceinline__ int64_t wave_inclusive_scan64(int64_t x, int lane) {
#pragma unroll
    for (int d = 1; d < kWave; d <<= 1) {
        const int64_t y = __shfl_up(x, d);
        if (lane >= d) x += y;
    }
    return x;
}

// pieces of a row: 0 for a whole row (and for a negative degree), ceil(deg / chunk) for a long one
__device__ __forceinline__ int64_t plan_pieces(int64_t deg, int32_t chunk) { return deg > chunk ? (deg + chunk - 1) / chunk : 0; }

// tile[3 tile + {0, 1, 2}] = the tile's long rows, pieces, rows with indptr[r + 1] < indptr[r]
__global__ __launch_bounds__(kBlock) void plan_tile_kernel(const int32_t* __restrict__ indptr, int64_t n_rows, int32_t chunk, uint32_t* __restrict__ keys,
                                                           int32_t* __restrict__ rows, int64_t* __restrict__ tile) {
    __shared__ int64_t part[4][3];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t start = (int64_t)blockIdx.x * kPlanTile;
    int64_t mine[3] = {0, 0, 0};
#pragma unroll
    for (int e = 0; e < kPlanRows; ++e) {
        const int64_t r = start + e * kBlock + tid;
        if (r < n_rows) {
            const int64_t deg = (int64_t)indptr[r + 1] - indptr[r];
            const bool whole = deg >= 0 && deg <= chunk;
            keys[r] = whole ? (uint32_t)(chunk - deg) : (uint32_t)chunk + 1u;
            rows[r] = (int32_t)r;
            mine[0] += deg > chunk, mine[1] += plan_pieces(deg, chunk), mine[2] += deg < 0;
        }
    }
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int64_t s = wave_inclusive_scan64(mine[q], lane);
        if (lane == 63) part[w][q] = s;
    }
    __syncthreads();
    if (tid < 3) tile[(int64_t)blockIdx.x * 3 + tid] = part[0][tid] + part[1][tid] + part[2][tid] + part[3][tid];
}

// tile[] -> its exclusive prefix over the tiles; sizes = {n_long, n_slots, n_bad}
__global__ __launch_bounds__(kBlock) void plan_tile_scan_kernel(int64_t* __restrict__ tile, int64_t tiles, int64_t* __restrict__ sizes) {
    __shared__ int64_t part[4][3], carry[3];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    if (tid < 3) carry[tid] = 0;
    __syncthreads();
    for (int64_t base = 0; base < tiles; base += kBlock) {
        const int64_t k = base + tid;
        int64_t v[3], inc[3];
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            v[q] = k < tiles ? tile[k * 3 + q] : 0;
            inc[q] = wave_inclusive_scan64(v[q], lane);
            if (lane == 63) part[w][q] = inc[q];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            int64_t before = carry[q];
            for (int u = 0; u < w; ++u) before += part[u][q];
            inc[q] += before;
            if (k < tiles) tile[k * 3 + q] = inc[q] - v[q];
        }
        __syncthreads();
        if (tid == kBlock - 1) carry[0] = inc[0], carry[1] = inc[1], carry[2] = inc[2];
        __syncthreads();
    }
    if (tid < 3) sizes[tid] = carry[tid];
}

// items[n_slots + i] = (r, indptr[r], indptr[r + 1], -1), r = the i-th row of the sort (the whole rows come first); long_ptr[n_long] = n_slots
__global__ __launch_bounds__(kBlock) void plan_fill_whole_kernel(const int32_t* __restrict__ indptr, int64_t n_rows, const int32_t* __restrict__ sorted,
                                                                 int64_t n_whole, int64_t n_long, int64_t n_slots, int4* __restrict__ items,
                                                                 int32_t* __restrict__ long_ptr) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i == 0) long_ptr[n_long] = (int32_t)n_slots;
    if (i >= n_whole) return;
    const int64_t r = sorted[i];
    if (r < 0 || r >= n_rows) return;
    items[n_slots + i] = make_int4((int32_t)r, indptr[r], indptr[r + 1], -1);
}

// long_rows[k] = r, long_ptr[k] = the first slot of r, for the long rows of the tile: thread t owns rows 8 t .. 8 t + 7 of it
__global__ __launch_bounds__(kBlock) void plan_fill_long_kernel(const int32_t* __restrict__ indptr, int64_t n_rows, int32_t chunk,
                                                                const int64_t* __restrict__ tile, int64_t n_long, int64_t n_slots,
                                                                int32_t* __restrict__ long_rows, int32_t* __restrict__ long_ptr) {
    __shared__ int64_t part[4][2];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t r0 = (int64_t)blockIdx.x * kPlanTile + (int64_t)tid * kPlanRows;
    int64_t pieces[kPlanRows], mine[2] = {0, 0};
#pragma unroll
    for (int e = 0; e < kPlanRows; ++e) {
        const int64_t r = r0 + e;
        pieces[e] = r < n_rows ? plan_pieces((int64_t)indptr[r + 1] - indptr[r], chunk) : 0;
        mine[0] += pieces[e] > 0, mine[1] += pieces[e];
    }
    int64_t inc[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        inc[q] = wave_inclusive_scan64(mine[q], lane);
        if (lane == 63) part[w][q] = inc[q];
    }
    __syncthreads();
    int64_t k = tile[(int64_t)blockIdx.x * 3] + inc[0] - mine[0], slot = tile[(int64_t)blockIdx.x * 3 + 1] + inc[1] - mine[1];
    for (int u = 0; u < w; ++u) k += part[u][0], slot += part[u][1];
#pragma unroll
    for (int e = 0; e < kPlanRows; ++e) {
        if (pieces[e] == 0) continue;
        if (k < n_long && slot < n_slots) long_rows[k] = (int32_t)(r0 + e), long_ptr[k] = (int32_t)slot;
        ++k, slot += pieces[e];
    }
}

// items[s] = (r, b, min(b + chunk, end), s): piece s - long_ptr[k] of the long row r = long_rows[k] that holds slot s
__global__ __launch_bounds__(kBlock) void plan_fill_slots_kernel(const int32_t* __restrict__ indptr, int64_t n_rows, int32_t chunk,
                                                                 const int32_t* __restrict__ long_rows, const int32_t* __restrict__ long_ptr,
                                                                 int64_t n_long, int64_t n_slots, int4* __restrict__ items) {
    const int64_t s = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (s >= n_slots) return;
    int64_t lo = 0, hi = n_long;                           // the last k with long_ptr[k] <= s
    while (hi - lo > 1) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (long_ptr[mid] <= s) lo = mid;
        else hi = mid;
    }
    const int64_t r = long_rows[lo];
    if (r < 0 || r >= n_rows) return;
    const int64_t end = indptr[r + 1], b = (int64_t)indptr[r] + (s - long_ptr[lo]) * chunk;
    items[s] = make_int4((int32_t)r, (int32_t)b, (int32_t)(b + chunk < end ? b + chunk : end), (int32_t)s);
}

// ------------------------------------------------------------------------------------------------ transpose
struct TransposeWorkspace {
    int64_t keys_a, keys_b, vals_a, vals_b, hist, total;           // byte offsets
};

static TransposeWorkspace transpose_workspace(int64_t nnz) {
    TransposeWorkspace w;
    int64_t o = 0;
    w.keys_a = o, o += plan_align(nnz * 4);
    w.keys_b = o, o += plan_align(nnz * 4);
    w.vals_a = o, o += plan_align(nnz * 4);
    w.vals_b = o, o += plan_align(nnz * 4);
    w.hist = o, o += plan_align(radix_tiles(nnz) * 256 * 4);
    w.total = o;
    return w;
}

static inline int transpose_passes(int64_t n_src) {               // 8 bits of the largest source id, n_src - 1, per pass
    int p = 1;
    while (p < 4 && ((n_src - 1) >> (8 * p)) > 0) ++p;
    return p;
}

__global__ __launch_bounds__(kBlock) void transpose_prep_kernel(const int32_t* __restrict__ indices, int64_t nnz, int64_t n_src, uint32_t* __restrict__ keys,
                                                                int32_t* __restrict__ vals, unsigned long long* __restrict__ n_bad) {
    const int64_t p = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    bool bad = false;
    if (p < nnz) {
        const int32_t s = indices[p];
        bad = s < 0 || s >= n_src;
        keys[p] = bad ? 0u : (uint32_t)s;
        vals[p] = (int32_t)p;
    }
    const uint64_t m = __ballot(bad);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(n_bad, (unsigned long long)__popcll(m));
}

// indices_r[k] = the row of `indptr` that holds position eid_r[k];  indptr_r[s] = the first sorted entry whose source is not below s
__global__ __launch_bounds__(kBlock) void transpose_finish_kernel(const int32_t* __restrict__ indptr, int64_t n_dst, int64_t n_src, int64_t nnz,
                                                                  const uint32_t* __restrict__ keys, const int32_t* __restrict__ eid_r,
                                                                  int32_t* __restrict__ indices_r, int32_t* __restrict__ indptr_r) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < nnz) {
        const int64_t p = eid_r[i];
        int64_t lo = 0, hi = n_dst;                        // the last row r < n_dst with indptr[r] <= p (rows without entries are skipped)
        while (hi - lo > 1) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (indptr[mid] <= p) lo = mid;
            else hi = mid;
        }
        indices_r[i] = (int32_t)lo;
    }
    if (i <= n_src) {
        int64_t lo = 0, hi = nnz;                          // the first k with keys[k] >= i
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if ((int64_t)keys[mid] < i) lo = mid + 1;
            else hi = mid;
        }
        indptr_r[i] = (int32_t)lo;
    }
}

static int plan_device_check(const int32_t* indptr, int64_t n_rows, int32_t chunk) {
    BOT_REQUIRE(indptr != nullptr, BOT_E_NULL, "row plan: indptr is NULL");
    BOT_REQUIRE(n_rows >= 0 && n_rows < INT32_MAX, BOT_E_RANGE, "row plan: n_rows=%lld out of range", (long long)n_rows);
    BOT_REQUIRE(chunk >= 1, BOT_E_RANGE, "row plan: chunk=%d must be >= 1", chunk);
    BOT_REQUIRE(chunk <= kPlanMaxChunk, BOT_E_RANGE, "row plan: the device planner takes chunk <= %d, got %d (use the host planner)", kPlanMaxChunk, chunk);
    return 0;
}

}  // namespace bot

extern "C" int64_t bot_row_plan_device_workspace_bytes(int64_t n_rows) {
    if (n_rows < 0 || n_rows >= INT32_MAX) return -1;
    return bot::plan_workspace(n_rows).total;
}

extern "C" int bot_row_plan_size_device(const int32_t* indptr, int64_t n_rows, int32_t chunk, void* workspace, int64_t workspace_bytes, int64_t* sizes,
                                        bot_stream_t stream) {
    using namespace bot;
    if (int rc = plan_device_check(indptr, n_rows, chunk)) return rc;
    BOT_REQUIRE(sizes != nullptr, BOT_E_NULL, "row plan: sizes is NULL");
    if (n_rows == 0) return 0;                             // nothing is launched: the empty plan
    const PlanWorkspace ws = plan_workspace(n_rows);
    BOT_REQUIRE(workspace != nullptr, BOT_E_NULL, "row plan: workspace is NULL");
    BOT_REQUIRE(workspace_bytes >= ws.total, BOT_E_RANGE, "row plan: workspace of %lld bytes, bot_row_plan_device_workspace_bytes asks for %lld",
                (long long)workspace_bytes, (long long)ws.total);
    BOT_REQUIRE(aligned(workspace, 8) && aligned(sizes, 8), BOT_E_ALIGN, "row plan: workspace / sizes is not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)workspace;
    uint32_t *ka = (uint32_t*)(base + ws.keys_a), *kb = (uint32_t*)(base + ws.keys_b), *hist = (uint32_t*)(base + ws.hist);
    int32_t *ra = (int32_t*)(base + ws.rows_a), *rb = (int32_t*)(base + ws.rows_b);
    int64_t* tile = (int64_t*)(base + ws.tile);
    set_kernel("plan_tile_kernel");
    hipLaunchKernelGGL(plan_tile_kernel, dim3((unsigned)ws.tiles), dim3(kBlock), 0, st, indptr, n_rows, chunk, ka, ra, tile);
    hipLaunchKernelGGL(plan_tile_scan_kernel, dim3(1), dim3(kBlock), 0, st, tile, ws.tiles, sizes);
    for (int pass = 0; pass < plan_passes(chunk); ++pass) {
        radix_pass<int32_t>(ka, ra, n_rows, 1, 8 * pass, hist, kb, rb, st);
        uint32_t* tk = ka;
        ka = kb, kb = tk;
        int32_t* tr = ra;
        ra = rb, rb = tr;
    }
    return hip_status("row plan (size) launch");
}

extern "C" int bot_row_plan_fill_device(const int32_t* indptr, int64_t n_rows, int32_t chunk, const void* workspace, int64_t workspace_bytes,
                                        int64_t n_items, int64_t n_long, int64_t n_slots, int32_t* items, int32_t* long_rows, int32_t* long_ptr,
                                        bot_stream_t stream) {
    using namespace bot;
    if (int rc = plan_device_check(indptr, n_rows, chunk)) return rc;
    BOT_REQUIRE(long_ptr != nullptr && (items != nullptr || n_rows == 0), BOT_E_NULL, "row plan: output pointer is NULL");
    BOT_REQUIRE(n_long >= 0 && n_long <= n_rows && n_slots >= 2 * n_long && (n_long > 0 || n_slots == 0) && n_items == n_rows - n_long + n_slots,
                BOT_E_PLAN, "row plan: n_items=%lld n_long=%lld n_slots=%lld do not belong to a plan of %lld rows", (long long)n_items, (long long)n_long,
                (long long)n_slots, (long long)n_rows);
    BOT_REQUIRE(n_items < INT32_MAX, BOT_E_RANGE, "row plan: n_items=%lld out of range", (long long)n_items);
    if (n_rows == 0) return 0;                             // nothing is launched (the caller's long_ptr = {0})
    BOT_REQUIRE(long_rows != nullptr || n_long == 0, BOT_E_NULL, "row plan: long_rows is NULL but long rows exist");
    const PlanWorkspace ws = plan_workspace(n_rows);
    BOT_REQUIRE(workspace != nullptr, BOT_E_NULL, "row plan: workspace is NULL");
    BOT_REQUIRE(workspace_bytes >= ws.total, BOT_E_RANGE, "row plan: workspace of %lld bytes, bot_row_plan_device_workspace_bytes asks for %lld",
                (long long)workspace_bytes, (long long)ws.total);
    BOT_REQUIRE(aligned(workspace, 8) && aligned(items, 16), BOT_E_ALIGN, "row plan: workspace (8 bytes) / items (16 bytes) is not aligned");
    hipStream_t st = (hipStream_t)stream;
    const char* base = (const char*)workspace;
    const int32_t* sorted = (const int32_t*)(base + ((plan_passes(chunk) & 1) ? ws.rows_b : ws.rows_a));
    const int64_t* tile = (const int64_t*)(base + ws.tile);
    const int64_t n_whole = n_rows - n_long;
    set_kernel("plan_fill_whole_kernel");
    hipLaunchKernelGGL(plan_fill_whole_kernel, dim3(launch_grid(n_whole, kBlock, INT32_MAX)), dim3(kBlock), 0, st, indptr, n_rows, sorted, n_whole, n_long,
                       n_slots, (int4*)items, long_ptr);
    if (n_long > 0) {
        hipLaunchKernelGGL(plan_fill_long_kernel, dim3((unsigned)ws.tiles), dim3(kBlock), 0, st, indptr, n_rows, chunk, tile, n_long, n_slots, long_rows,
                           long_ptr);
        hipLaunchKernelGGL(plan_fill_slots_kernel, dim3(launch_grid(n_slots, kBlock, INT32_MAX)), dim3(kBlock), 0, st, indptr, n_rows, chunk, long_rows,
                           long_ptr, n_long, n_slots, (int4*)items);
    }
    return hip_status("row plan (fill) launch");
}

extern "C" int64_t bot_csc_transpose_workspace_bytes(int64_t nnz) {
    if (nnz < 0 || nnz >= INT32_MAX) return -1;
    return bot::transpose_workspace(nnz).total;
}

extern "C" int bot_csc_transpose_i32(const int32_t* indptr, const int32_t* indices, int64_t n_dst, int64_t n_src, int64_t nnz, int32_t* indptr_r,
                                     int32_t* indices_r, int32_t* eid_r, int64_t* n_bad, void* workspace, int64_t workspace_bytes,
                                     bot_stream_t stream) {
    using namespace bot;
    BOT_REQUIRE(indptr != nullptr && indptr_r != nullptr && n_bad != nullptr, BOT_E_NULL, "csc transpose: indptr / indptr_r / n_bad is NULL");
    BOT_REQUIRE(nnz >= 0 && nnz < INT32_MAX && n_src >= 0 && n_src < INT32_MAX && n_dst >= 0 && n_dst < INT32_MAX && (nnz == 0 || (n_dst > 0 && n_src > 0)),
                BOT_E_RANGE, "csc transpose: n_dst=%lld n_src=%lld nnz=%lld out of range (below 2^31 - 1; entries need rows on both sides)",
                (long long)n_dst, (long long)n_src, (long long)nnz);
    if (nnz == 0) return 0;                                // nothing is launched: indptr_r is the caller's zeros
    BOT_REQUIRE(indices != nullptr && indices_r != nullptr && eid_r != nullptr && workspace != nullptr, BOT_E_NULL,
                "csc transpose: indices / indices_r / eid_r / workspace is NULL");
    const TransposeWorkspace ws = transpose_workspace(nnz);
    BOT_REQUIRE(workspace_bytes >= ws.total, BOT_E_RANGE, "csc transpose: workspace of %lld bytes, bot_csc_transpose_workspace_bytes asks for %lld",
                (long long)workspace_bytes, (long long)ws.total);
    BOT_REQUIRE(aligned(workspace, 8) && aligned(n_bad, 8), BOT_E_ALIGN, "csc transpose: workspace / n_bad is not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    set_kernel("transpose_finish_kernel");
    hipError_t e = hipMemsetAsync(n_bad, 0, sizeof(int64_t), st);
    BOT_REQUIRE(e == hipSuccess, (int)e, "csc transpose: %s", hipGetErrorString(e));
    char* base = (char*)workspace;
    uint32_t *ka = (uint32_t*)(base + ws.keys_a), *kb = (uint32_t*)(base + ws.keys_b), *hist = (uint32_t*)(base + ws.hist);
    int32_t *va = (int32_t*)(base + ws.vals_a), *vb = (int32_t*)(base + ws.vals_b);
    hipLaunchKernelGGL(transpose_prep_kernel, dim3(launch_grid(nnz, kBlock, INT32_MAX)), dim3(kBlock), 0, st, indices, nnz, n_src, ka, va,
                       (unsigned long long*)n_bad);
    const int passes = transpose_passes(n_src);
    for (int pass = 0; pass < passes; ++pass) {
        radix_pass<int32_t>(ka, va, nnz, 1, 8 * pass, hist, kb, pass == passes - 1 ? eid_r : vb, st);     // the last pass lands in eid_r
        uint32_t* tk = ka;
        ka = kb, kb = tk;
        int32_t* tv = va;
        va = vb, vb = tv;
    }
    const int64_t m = nnz > n_src + 1 ? nnz : n_src + 1;
    hipLaunchKernelGGL(transpose_finish_kernel, dim3(launch_grid(m, kBlock, INT32_MAX)), dim3(kBlock), 0, st, indptr, n_dst, n_src, nnz, ka, eid_r,
                       indices_r, indptr_r);
    return hip_status("csc transpose launch");
}
