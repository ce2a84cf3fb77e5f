// GraphSAINT node sets for subgraph mini-batches (Zeng et al., ICLR 2020; DGL's SAINTSampler "walk" / "node"), gfx950: the walks.
//
// Walk i starts at a root (root_mode 0: a uniform draw from `nids`, with replacement; root_mode 1: the source of a uniformly
// drawn edge, i.e. a node drawn in proportion to its out-degree) and takes `length` steps, each to a uniformly drawn in-neighbour
// of the node it stands on (a CSC row of the parent; a node without in-edges stays where it is).  It follows in-edges backwards
// because the node reached sends a message to the node it was reached from: that edge is in the induced subgraph.  The draw of
// walk i at step t is umulhi64(x, range) with x = Philox::word64(seed, i, t), the first 64 bits of Philox4x32-10(seed, counter =
// i << 32 | t) as floyd_draw (sampling.hip) takes them: bias below 2^-32, and a pure function of (i, t, seed) - independent of the launch shape
// and of the run.
//
// One lane per walk, one wave of 64 per workgroup so that a batch's 10^3 - 10^5 walks spread over the CUs: the launch is bound by
// latency, two dependent loads per step (indptr[v] and indptr[v + 1] from one line, then indices[...]), every walk in flight
// together.  The distinct nodes of the trace are listed by bot_saint_nodes_*_i32 (sampling.hip, on the block builder's scan).
#include "common.h"

namespace bot {

__device__ __forceinline__ uint64_t saint_draw(uint64_t seed, int64_t walk, int32_t step, uint64_t range) {
    return __umul64hi(Philox::word64(seed, (uint32_t)walk, (uint32_t)step), range);
}

__global__ __launch_bounds__(kWave) void saint_walk_kernel(const int32_t* __restrict__ indptr, const int32_t* __restrict__ indices, int64_t n_rows,
                                                           int64_t nnz, const int32_t* __restrict__ nids, int64_t n_nids, int64_t n_roots,
                                                           int32_t length, int32_t root_mode, uint64_t seed, int32_t* __restrict__ trace) {
    for (int64_t i = (int64_t)blockIdx.x * kWave + threadIdx.x; i < n_roots; i += (int64_t)gridDim.x * kWave) {
        int32_t v;
        if (root_mode == 1) v = indices[saint_draw(seed, i, 0, (uint64_t)nnz)];
        else if (nids) v = nids[saint_draw(seed, i, 0, (uint64_t)n_nids)];
        else v = (int32_t)saint_draw(seed, i, 0, (uint64_t)n_rows);
        int32_t* out = trace + i * ((int64_t)length + 1);
        out[0] = v;
        for (int32_t t = 1; t <= length; ++t) {
            if (v >= 0 && v < n_rows) {               // an id outside the parent's rows (a bad `nids`) has no row to read: it stays
                const int32_t base = indptr[v], deg = indptr[v + 1] - base;
                if (deg > 0) v = indices[base + (int64_t)saint_draw(seed, i, t, (uint64_t)deg)];
            }
            out[t] = v;
        }
    }
}

}  // namespace bot

extern "C" int bot_saint_walk_i32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* nids, int64_t n_nids,
                                  int64_t n_roots, int32_t length, int32_t root_mode, uint64_t seed, int32_t* trace, bot_stream_t stream) {
    using namespace bot;
    BOT_REQUIRE(n_rows >= 0 && n_rows < (1ll << 31) && nnz >= 0 && nnz < (1ll << 31) && n_nids >= 0 && n_roots >= 0 && n_roots < (1ll << 31) && length >= 0 &&
                    n_roots * ((int64_t)length + 1) < (1ll << 31),
                BOT_E_RANGE, "saint_walk: n_rows=%lld nnz=%lld n_nids=%lld n_roots=%lld length=%d (n_roots (length + 1) < 2^31)", (long long)n_rows,
                (long long)nnz, (long long)n_nids, (long long)n_roots, (int)length);
    BOT_REQUIRE(root_mode == 0 || (root_mode == 1 && nids == nullptr && nnz > 0), BOT_E_RANGE,
                "saint_walk: root_mode=%d (0: uniform over nids; 1: in proportion to out-degree, which takes no nids and at least one edge)",
                (int)root_mode);
    BOT_REQUIRE(indptr != nullptr, BOT_E_NULL, "saint_walk: indptr is NULL");
    if (n_roots == 0) return 0;
    BOT_REQUIRE(root_mode == 1 || (nids ? n_nids : n_rows) > 0, BOT_E_RANGE, "saint_walk: %lld roots asked of an empty node set", (long long)n_roots);
    BOT_REQUIRE(trace != nullptr && (nnz == 0 || indices != nullptr), BOT_E_NULL, "saint_walk: NULL indices / trace");
    set_kernel("saint_walk_kernel");
    hipLaunchKernelGGL(saint_walk_kernel, dim3(launch_grid(n_roots, kWave, 1 << 20)), dim3(kWave), 0, (hipStream_t)stream, indptr, indices,
                       n_rows, nnz, nids, n_nids, n_roots, length, root_mode, seed, trace);
    return hip_status("saint_walk launch");
}
