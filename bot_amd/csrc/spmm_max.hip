// Max-reduce sweep pair (include/bot_gnn.h "Max aggregation") for gfx950: the pool aggregator of GraphSAGE (Hamilton, Ying, Leskovec,
// NeurIPS 2017; bot_amd.nn.SAGEConv) and `update_all(fn.copy_u, fn.max)`.
//   forward   out[r,f] = max_k x[indices[k],f],  arg[r,f] = the smallest position k that attains it   (rows = destinations: the CSC)
//   backward  dx[u,f]  = sum_j dout[indices[j],f] * (arg[indices[j],f] == pos[j])                     (rows = sources: the CSR)
//
// The gather is the lane-group row sweep that sweep.h describes.  A row wider than the group's tile (64 lanes x VEC x 2) walks feature tiles; the
// ids are read again per tile (sequential, 4 bytes against a 4 F-byte row).
//
// Forward: every lane keeps the running (max, position) pair of its columns in registers and visits the neighbours in position order
// with a strict `>`, so the earliest position of a tie wins and -0.0 == +0.0 tie; the pair starts at (-inf, first position), so a row of
// -inf has a position too and a NaN never enters (a NaN compares false).  One plain store of each at the end.  The chunks of a long
// row leave their pairs in the workspace; spmm_max_combine_kernel (one thread per long row and column) folds them in slot order with
// the same strict `>` (slot order is position order) and applies the epilogue.  relu: out = max(m, 0) and arg = -1 where m <= 0 - `max_u relu(z_u) = relu(max_u z_u)`, so
// the [n_src, F] ReLU pass in front of the reduce and its backward are never run, and arg = -1 carries the gate to the backward.
//
// Backward: position, not source id, is what arg stores, so of two parallel edges exactly one matches.  Per out-edge two row gathers
// (dout and arg of the destination) and a select; the sum runs in position order in registers, long rows chunk by chunk into `partial`
// and through the slot-order combine.  No atomics in either direction: the bytes repeat from call to call.
//
// HBM model: forward 4 * [E * (1 + F) + 2 * n_rows * F] bytes (ids and source rows per edge; out and arg per row) - the sum sweep's plus
// the arg store; backward 4 * [E * (2 + 2 F) + n_src * F] (ids, positions, a dout row and an arg row per edge; dx per row) - twice the
// transposed sum sweep's gather.
#include "sweep.h"

#include <initializer_list>
#include <math.h>

namespace bot {

template <int VEC>
__device__ __forceinline__ void ivload(int (&r)[VEC], const int32_t* p) {
    typedef int iv __attribute__((ext_vector_type(VEC)));
    const iv v = *reinterpret_cast<const iv*>(p);
#pragma unroll
    for (int t = 0; t < VEC; ++t) r[t] = v[t];
}
template <>
__device__ __forceinline__ void ivload<1>(int (&r)[1], const int32_t* p) { r[0] = *p; }

template <int VEC>
__device__ __forceinline__ void ivstore(int32_t* p, const int (&r)[VEC]) {
    typedef int iv __attribute__((ext_vector_type(VEC)));
    iv v;
#pragma unroll
    for (int t = 0; t < VEC; ++t) v[t] = r[t];
    *reinterpret_cast<iv*>(p) = v;
}
template <>
__device__ __forceinline__ void ivstore<1>(int32_t* p, const int (&r)[1]) { *p = r[0]; }

struct MaxArgs {
    const int32_t* indices;
    const int4* items;
    int64_t n_items;
    const float* x;
    int64_t ldx;
    float* out;
    int64_t ldo;
    int32_t* arg;
    int64_t lda;
    int32_t F;
    int32_t relu;
    float* pval;    // [n_slots, F] chunk maxima
    int32_t* ppos;  // [n_slots, F] their positions
};

// The epilogue of one (max, position) pair: an empty row (p < 0) is (0, -1); relu gates m <= 0 to (0, -1).
__device__ __forceinline__ void max_finish(bool relu, float& m, int& p) {
    if (p < 0 || (relu && !(m > 0.f))) {
        m = 0.f;
        p = -1;
    }
}

template <int VEC, int LANES, int NCHUNK>
__global__ __launch_bounds__(kBlock) void spmm_max_kernel(MaxArgs a) {
    constexpr int U = 4;
    constexpr int TILE = LANES * VEC * NCHUNK;
    const int lane = threadIdx.x % LANES;
    const int64_t item = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / LANES;
    if (item >= a.n_items) return;  // whole groups leave together
    const RowItem it = load_item<LANES>(a.items, item);
    const bool relu = a.relu != 0;
    for (int col0 = 0; col0 < a.F; col0 += TILE) {  // groups narrower than a wavefront have one tile (MaxLaunch)
        const ColTile<VEC, LANES, NCHUNK> tile(col0, lane, a.F);
        float mx[NCHUNK][VEC];
        int am[NCHUNK][VEC];
#pragma unroll
        for (int c = 0; c < NCHUNK; ++c)
#pragma unroll
            for (int t = 0; t < VEC; ++t) {
                mx[c][t] = -INFINITY;
                am[c][t] = it.beg < it.end ? it.beg : -1;
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
                    const float* p = a.x + (int64_t)s * a.ldx;
#pragma unroll
                    for (int c = 0; c < NCHUNK; ++c) vload<VEC>(v[u][c], p + tile.off[c]);
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int c = 0; c < NCHUNK; ++c)
#pragma unroll
                        for (int t = 0; t < VEC; ++t)
                            if (v[u][c][t] > mx[c][t]) {
                                mx[c][t] = v[u][c][t];
                                am[c][t] = k0 + i + u;
                            }
            }
            for (; i < cnt; ++i) {
                const int s = group_bcast<LANES>(idx, i);
                const float* p = a.x + (int64_t)s * a.ldx;
                float v[NCHUNK][VEC];
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c) vload<VEC>(v[c], p + tile.off[c]);
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c)
#pragma unroll
                    for (int t = 0; t < VEC; ++t)
                        if (v[c][t] > mx[c][t]) {
                            mx[c][t] = v[c][t];
                            am[c][t] = k0 + i;
                        }
            }
        }
        if (it.slot >= 0) {  // a chunk of a long row: the raw pair, folded by spmm_max_combine_kernel
            float* pv = a.pval + (int64_t)it.slot * a.F;
            int32_t* pp = a.ppos + (int64_t)it.slot * a.F;
#pragma unroll
            for (int c = 0; c < NCHUNK; ++c)
                if (tile.act[c]) {
                    vstore<VEC>(pv + tile.off[c], mx[c]);
                    ivstore<VEC>(pp + tile.off[c], am[c]);
                }
            continue;
        }
#pragma unroll
        for (int c = 0; c < NCHUNK; ++c)
            if (tile.act[c]) {
#pragma unroll
                for (int t = 0; t < VEC; ++t) max_finish(relu, mx[c][t], am[c][t]);
                vstore<VEC>(a.out + (int64_t)it.row * a.ldo + tile.off[c], mx[c]);
                ivstore<VEC>(a.arg + (int64_t)it.row * a.lda + tile.off[c], am[c]);
            }
    }
}

// One thread per (long row, column), as spmm_combine_kernel: the chunks' pairs are folded in slot order (= position order) with the
// sweep's strict `>`, four slots' loads in flight, then the row's epilogue.
__global__ __launch_bounds__(kBlock) void spmm_max_combine_kernel(MaxArgs a, const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long) {
    const int64_t gid = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (gid >= n_long * a.F) return;
    const int64_t i = gid / a.F;
    const int c = (int)(gid - i * a.F);
    const int row = long_rows[i], p1 = long_ptr[i + 1];
    int s = long_ptr[i];
    float m = -INFINITY;
    int p = -1;
    if (s < p1) {  // the first chunk's pair is taken as it is: a row of -inf keeps its first position
        m = a.pval[(int64_t)s * a.F + c];
        p = a.ppos[(int64_t)s * a.F + c];
        ++s;
    }
    for (; s + 4 <= p1; s += 4) {
        float v[4];
        int q[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v[j] = a.pval[(int64_t)(s + j) * a.F + c];
            q[j] = a.ppos[(int64_t)(s + j) * a.F + c];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (v[j] > m) {
                m = v[j];
                p = q[j];
            }
    }
    for (; s < p1; ++s) {
        const float v = a.pval[(int64_t)s * a.F + c];
        const int q = a.ppos[(int64_t)s * a.F + c];
        if (v > m) {
            m = v;
            p = q;
        }
    }
    max_finish(a.relu != 0, m, p);
    a.out[(int64_t)row * a.ldo + c] = m;
    a.arg[(int64_t)row * a.lda + c] = p;
}

struct MaxBwdArgs {
    const int32_t* indices;
    const int32_t* pos;
    const int4* items;
    int64_t n_items;
    const float* dout;
    int64_t ldd;
    const int32_t* arg;
    int64_t lda;
    float* dx;
    int64_t ldx;
    int32_t F;
    float* partial;  // [n_slots, F] chunk sums
};

template <int VEC, int LANES, int NCHUNK>
__global__ __launch_bounds__(kBlock) void spmm_max_bwd_kernel(MaxBwdArgs a) {
    constexpr int U = 4;
    constexpr int TILE = LANES * VEC * NCHUNK;
    const int lane = threadIdx.x % LANES;
    const int64_t item = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / LANES;
    if (item >= a.n_items) return;  // whole groups leave together
    const RowItem it = load_item<LANES>(a.items, item);
    for (int col0 = 0; col0 < a.F; col0 += TILE) {
        const ColTile<VEC, LANES, NCHUNK> tile(col0, lane, a.F);
        float acc[NCHUNK][VEC] = {};
        for (int k0 = it.beg; k0 < it.end; k0 += LANES) {
            const int k = k0 + lane;
            int idx = 0, pk = -2;  // -2: no arg entry equals it
            if (k < it.end) {
                idx = a.indices[k];
                pk = a.pos[k];
            }
            const int cnt = min(LANES, it.end - k0);
            int i = 0;
            for (; i + U <= cnt; i += U) {
                float d[U][NCHUNK][VEC];
                int g[U][NCHUNK][VEC], pp[U];
#pragma unroll
                for (int u = 0; u < U; ++u) {
                    const int s = group_bcast<LANES>(idx, i + u);
                    pp[u] = group_bcast<LANES>(pk, i + u);
                    const float* pd = a.dout + (int64_t)s * a.ldd;
                    const int32_t* pa = a.arg + (int64_t)s * a.lda;
#pragma unroll
                    for (int c = 0; c < NCHUNK; ++c) {
                        vload<VEC>(d[u][c], pd + tile.off[c]);
                        ivload<VEC>(g[u][c], pa + tile.off[c]);
                    }
                }
#pragma unroll
                for (int u = 0; u < U; ++u)
#pragma unroll
                    for (int c = 0; c < NCHUNK; ++c)
#pragma unroll
                        for (int t = 0; t < VEC; ++t) acc[c][t] += g[u][c][t] == pp[u] ? d[u][c][t] : 0.f;
            }
            for (; i < cnt; ++i) {
                const int s = group_bcast<LANES>(idx, i);
                const int p1 = group_bcast<LANES>(pk, i);
                const float* pd = a.dout + (int64_t)s * a.ldd;
                const int32_t* pa = a.arg + (int64_t)s * a.lda;
                float d[NCHUNK][VEC];
                int g[NCHUNK][VEC];
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c) {
                    vload<VEC>(d[c], pd + tile.off[c]);
                    ivload<VEC>(g[c], pa + tile.off[c]);
                }
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c)
#pragma unroll
                    for (int t = 0; t < VEC; ++t) acc[c][t] += g[c][t] == p1 ? d[c][t] : 0.f;
            }
        }
        tile.store(sum_row(it, a.dx, a.ldx, a.partial, a.F), acc);
    }
}

template <bool BWD, class Args>
struct MaxLaunch {
    const Args& a;
    hipStream_t st;
    template <int VEC, int LANES, int NCHUNK>
    void run() const {
        const int64_t blocks = (a.n_items * LANES + kBlock - 1) / kBlock;
        if (blocks == 0) return;
        if constexpr (BWD) {
            set_kernel("bot::spmm_max_bwd_kernel<%d,%d,%d>", VEC, LANES, NCHUNK);
            hipLaunchKernelGGL((spmm_max_bwd_kernel<VEC, LANES, NCHUNK>), dim3((unsigned)blocks), dim3(kBlock), 0, st, a);
        } else {
            set_kernel("bot::spmm_max_kernel<%d,%d,%d>", VEC, LANES, NCHUNK);
            hipLaunchKernelGGL((spmm_max_kernel<VEC, LANES, NCHUNK>), dim3((unsigned)blocks), dim3(kBlock), 0, st, a);
        }
    }
    template <int VEC>
    void wide(int) const {
        run<VEC, 64, 2>();  // wider rows walk tiles of 128 lanes
    }
};

}  // namespace bot

extern "C" {

int bot_spmm_max_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                     const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, int64_t n_slots, const float* x, int64_t ldx, int32_t F,
                     int32_t relu, float* out, int64_t ldo, int32_t* arg, int64_t lda, void* workspace, bot_stream_t stream) {
    using namespace bot;
    (void)indptr;
    if (int rc = check_plan_sizes("spmm_max", n_rows, nnz, n_items, n_long, n_slots)) return rc;
    BOT_REQUIRE(F >= 1, BOT_E_RANGE, "spmm_max: F=%d (>= 1)", F);
    if (n_rows == 0) return 0;
    if (int rc = check_plan("spmm_max", items, "items/x/out/arg", x && out && arg, nnz, "indices", indices, n_long,
                            "long_rows/long_ptr/workspace", long_rows && long_ptr && workspace))
        return rc;
    BOT_REQUIRE(n_long == 0 || n_slots > 0, BOT_E_RANGE, "spmm_max: long rows without slots");
    BOT_REQUIRE(out != x, BOT_E_RANGE, "spmm_max: out aliases x");
    BOT_REQUIRE(ldx >= F && ldo >= F && lda >= F, BOT_E_RANGE, "spmm_max: row strides smaller than F=%d (ldx=%lld ldo=%lld lda=%lld)", F,
                (long long)ldx, (long long)ldo, (long long)lda);
    BOT_REQUIRE(aligned(x, 4) && aligned(out, 4) && aligned(arg, 4) && aligned(items, 16) && aligned(workspace, 16), BOT_E_ALIGN,
                "spmm_max: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    float* pval = static_cast<float*>(workspace);
    const MaxArgs a{indices, reinterpret_cast<const int4*>(items), n_items, x, ldx, out, ldo, arg, lda, F, relu,
                    pval, pval ? reinterpret_cast<int32_t*>(pval + n_slots * F) : nullptr};
    const int vec = pick_vec(F, {ldx, ldo, lda}, {x, out, arg});  // (the workspace: 16-byte base, slot rows of F floats)
    dispatch_sweep(MaxLaunch<false, MaxArgs>{a, st}, F, vec);
    if (int rc = hip_status("spmm_max launch")) return rc;
    if (n_long > 0) {
        hipLaunchKernelGGL(spmm_max_combine_kernel, dim3((unsigned)((n_long * F + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, a, long_rows,
                           long_ptr, n_long);
        if (int rc = hip_status("spmm_max combine launch")) return rc;
    }
    return 0;
}

int bot_spmm_max_bwd_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                         const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, const int32_t* pos, const float* dout, int64_t ldd,
                         const int32_t* arg, int64_t lda, int32_t F, float* dx, int64_t ldx, float* partial, bot_stream_t stream) {
    using namespace bot;
    (void)indptr;
    if (int rc = check_plan_sizes("spmm_max_bwd", n_rows, nnz, n_items, n_long)) return rc;
    BOT_REQUIRE(F >= 1, BOT_E_RANGE, "spmm_max_bwd: F=%d (>= 1)", F);
    if (n_rows == 0) return 0;
    if (int rc = check_plan("spmm_max_bwd", items, "items/dx", dx, nnz, "indices/pos/dout/arg", indices && pos && dout && arg, n_long,
                            "long_rows/long_ptr/partial", long_rows && long_ptr && partial))
        return rc;
    BOT_REQUIRE(dx != dout, BOT_E_RANGE, "spmm_max_bwd: dx aliases dout");
    BOT_REQUIRE(ldd >= F && lda >= F && ldx >= F, BOT_E_RANGE, "spmm_max_bwd: row strides smaller than F=%d (ldd=%lld lda=%lld ldx=%lld)", F,
                (long long)ldd, (long long)lda, (long long)ldx);
    BOT_REQUIRE(aligned(dout, 4) && aligned(arg, 4) && aligned(dx, 4) && aligned(items, 16) && aligned(partial, 16), BOT_E_ALIGN,
                "spmm_max_bwd: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    const MaxBwdArgs a{indices, pos, reinterpret_cast<const int4*>(items), n_items, dout, ldd, arg, lda, dx, ldx, F, partial};
    const int vec = pick_vec(F, {ldd, lda, ldx}, {dout, arg, dx});
    dispatch_sweep(MaxLaunch<true, MaxBwdArgs>{a, st}, F, vec);
    if (int rc = hip_status("spmm_max_bwd launch")) return rc;
    if (n_long > 0) {
        launch_sum_combine(partial, F, dx, ldx, long_rows, long_ptr, n_long, st);
        if (int rc = hip_status("spmm_max_bwd combine launch")) return rc;
    }
    return 0;
}

}  // extern "C"
