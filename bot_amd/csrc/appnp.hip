// One step of personalised-PageRank propagation (include/bot_gnn.h "APPNP step") for gfx950, forward or backward:
//   q_k = pos ? pos[k] : k;   m_k = p == 0 ? 1 : (keep(seed, step, q_k) ? 1 / (1 - p) : 0)
//   s   = sum_{k in row v} src_scale[indices[k]] * ew[k] * m_k * y[indices[k], :]
//   o   = a * dst_scale[v] * s + b * y0[v, :];   acc_out[v, :] = acc_in[v, :] + o;   out[v, :] = out_scale[v] * o
//
// It is propagate.hip's sweep (the lane-group row sweep of sweep.h, the same lane-group widths, the same long-row combine) with
// what training needs: the edge-drop mask is REGENERATED from a counter - keep(seed, step, q) is word q & 3 of Philox4x32-10 under the
// key `seed` at the counter step << 32 | q >> 2, kept iff (w >> 8) * 2^-24 >= p (dense.hip's drop_factors rule) - so neither the forward
// nor the backward stores a mask, and the backward, a sweep over the CSR, reaches the forward's bit of an edge through pos = csr2csc,
// one more streamed word per edge read by the lane that reads indices[k], as ew[k] is.  The mask is a function of (seed, step, q)
// alone, never of the lane layout.  A dropped position contributes NOTHING: its id travels as -1, its row is not gathered (with 64-lane
// groups the id sits in an SGPR and a scalar branch skips the loads; narrower groups predicate them per lane - spmm.hip's zero-weight
// skip) and its factor is 0, so a NaN or inf in a dropped source row or weight never reaches the sum.  The propagation is linear, so its
// backward needs no activation: acc_out = acc_in + o sums the steps' gradients for d h0 in the epilogue of the lanes that hold the row.
//
// The multiplications by absent operands do not happen: with p == 0, ew == NULL, pos == NULL, acc_out == NULL and y0 given the
// instances are prop_step_kernel's arithmetic, and `out` is bit for bit bot_propagate_step_f32's without clamp, fixed rows and row_abs.
// Plain stores only: no atomics, every element of acc is read and written by one lane, the bytes repeat from call to call.
//
// HBM model per sweep: 4 * [E_kept * C + E * (1 + [src_scale] + [ew] + [pos]) + N * C * (1 + [y0] + 2 * [acc])] bytes (the gathered
// rows of the kept edges; ids and the optional per-edge words; out, y0 and acc in + out per node).  The Philox block is ten rounds per
// four positions, computed by one lane per position beside a gather of C floats: assumed negligible, not measured.
#include "sweep.h"

#include <initializer_list>

namespace bot {

struct AppnpArgs {
    const int32_t* indices;
    const int4* items;
    int64_t n_items;
    const float* y;
    int64_t ldy;
    const float* y0;
    int64_t ldy0;
    float* out;
    int64_t ldo;
    int32_t C;
    float a, b;
    const float* src_scale;
    const float* dst_scale;
    const float* out_scale;
    const float* acc_in;
    int64_t ldai;
    float* acc_out;
    int64_t ldao;
    float* partial;
    const float* ew;
    const int32_t* pos;
    float p, inv_keep;
    uint64_t seed;
    uint32_t step;
};

// whether position q of step `step` is kept: a function of (seed, step, q) only
__device__ __forceinline__ bool appnp_keep(uint64_t seed, uint32_t step, uint32_t q, float p) {
    uint32_t w[4];
    Philox::gen(seed, ((uint64_t)step << 32) | (q >> 2), w);
    const uint32_t r = (q & 2) ? ((q & 1) ? w[3] : w[2]) : ((q & 1) ? w[1] : w[0]);
    return ((r >> 8) * (1.0f / 16777216.0f)) >= p;
}

// The epilogue of VEC consecutive columns of row `row`: s holds the gathered sums on entry.  prop_finish's order of operations, without
// the clamp and the fixed rows; the sum into acc is one rounded add of its own.
template <int VEC>
__device__ __forceinline__ void appnp_finish(const AppnpArgs& a, int row, int col, float av, float osc, float (&s)[VEC]) {
    float r[VEC], ai[VEC];
    if (a.y0) vload<VEC>(r, a.y0 + (int64_t)row * a.ldy0 + col);
    if (a.acc_out) vload<VEC>(ai, a.acc_in + (int64_t)row * a.ldai + col);
#pragma unroll
    for (int t = 0; t < VEC; ++t) {
        const float o = a.y0 ? fmaf(av, s[t], a.b * r[t]) : __fmul_rn(av, s[t]);
        if (a.acc_out) ai[t] = __fadd_rn(ai[t], o);
        s[t] = o * osc;
    }
    if (a.acc_out) vstore<VEC>(a.acc_out + (int64_t)row * a.ldao + col, ai);
    vstore<VEC>(a.out + (int64_t)row * a.ldo + col, s);
}

template <int VEC, int LANES, int NCHUNK, bool EW, bool DROP>
__global__ __launch_bounds__(kBlock) void appnp_step_kernel(AppnpArgs a) {
    constexpr int U = 4;
    const int lane = threadIdx.x % LANES;
    const int64_t item = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / LANES;
    if (item >= a.n_items) return;  // whole groups leave together
    const RowItem it = load_item<LANES>(a.items, item);
    const int row = it.row;
    const ColTile<VEC, LANES, NCHUNK> tile(0, lane, a.C);
    float acc[NCHUNK][VEC] = {};
    for (int k0 = it.beg; k0 < it.end; k0 += LANES) {
        const int k = k0 + lane;
        int idx = 0;
        float sv = 1.f;
        if (k < it.end) {
            idx = a.indices[k];
            float wk = 1.f;
            if constexpr (EW) wk = a.ew[k];  // streamed beside the id: issued before the scale's dependent read
            uint32_t q = (uint32_t)k;
            if constexpr (DROP) {
                if (a.pos) q = (uint32_t)a.pos[k];  // the backward's word: the forward's (CSC) position of this edge
            }
            if (a.src_scale) sv = a.src_scale[idx];
            if constexpr (EW) sv *= wk;
            if constexpr (DROP) {
                if (appnp_keep(a.seed, a.step, q, a.p)) sv *= a.inv_keep;
                else idx = -1, sv = 0.f;  // dropped: no gather, no term
            }
        }
        const int cnt = min(LANES, it.end - k0);
        int i = 0;
        for (; i + U <= cnt; i += U) {
            float v[U][NCHUNK][VEC], ww[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int s = group_bcast<LANES>(idx, i + u);
                ww[u] = group_bcast<LANES>(sv, i + u);
                if (!DROP || s >= 0) {
                    const float* p = a.y + (int64_t)s * a.ldy;
#pragma unroll
                    for (int c = 0; c < NCHUNK; ++c) vload<VEC>(v[u][c], p + tile.off[c]);
                } else {
#pragma unroll
                    for (int c = 0; c < NCHUNK; ++c)
#pragma unroll
                        for (int t = 0; t < VEC; ++t) v[u][c][t] = 0.f;
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c)
#pragma unroll
                    for (int t = 0; t < VEC; ++t) acc[c][t] = fmaf(ww[u], v[u][c][t], acc[c][t]);
        }
        for (; i < cnt; ++i) {
            const int s = group_bcast<LANES>(idx, i);
            const float w1 = group_bcast<LANES>(sv, i);
            if (DROP && s < 0) continue;  // uniform over the group
            const float* p = a.y + (int64_t)s * a.ldy;
            float v[NCHUNK][VEC];
#pragma unroll
            for (int c = 0; c < NCHUNK; ++c) vload<VEC>(v[c], p + tile.off[c]);
#pragma unroll
            for (int c = 0; c < NCHUNK; ++c)
#pragma unroll
                for (int t = 0; t < VEC; ++t) acc[c][t] = fmaf(w1, v[c][t], acc[c][t]);
        }
    }
    if (it.slot >= 0) {  // a chunk of a long row: the raw sum, finished by appnp_combine_kernel
        tile.store(a.partial + (int64_t)it.slot * a.C, acc);
        return;
    }
    const float av = a.a * (a.dst_scale ? a.dst_scale[row] : 1.f);
    const float osc = a.out_scale ? a.out_scale[row] : 1.f;
#pragma unroll
    for (int c = 0; c < NCHUNK; ++c)
        if (tile.act[c]) appnp_finish<VEC>(a, row, tile.off[c], av, osc, acc[c]);
}

// One wavefront per long row: column c = lane, lane + 64, ...; the chunk sums are added in slot order, then the row's epilogue.
__global__ __launch_bounds__(kBlock) void appnp_combine_kernel(AppnpArgs a, const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long) {
    const int lane = threadIdx.x & 63;
    const int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    if (i >= n_long) return;  // whole waves leave together
    const int row = long_rows[i], p0 = long_ptr[i], p1 = long_ptr[i + 1];
    const float av = a.a * (a.dst_scale ? a.dst_scale[row] : 1.f);
    const float osc = a.out_scale ? a.out_scale[row] : 1.f;
    for (int c = lane; c < a.C; c += 64) {
        float s[1] = {0.f};
        int p = p0;
        for (; p + 4 <= p1; p += 4) {  // four loads in flight, added in slot order
            float v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = a.partial[(int64_t)(p + j) * a.C + c];
#pragma unroll
            for (int j = 0; j < 4; ++j) s[0] += v[j];
        }
        for (; p < p1; ++p) s[0] += a.partial[(int64_t)p * a.C + c];
        appnp_finish<1>(a, row, c, av, osc, s);
    }
}

template <bool EW, bool DROP>
struct AppnpLaunch {
    const AppnpArgs& a;
    hipStream_t st;
    template <int VEC, int LANES, int NCHUNK>
    void run() const {
        if constexpr (VEC * NCHUNK <= 16) {  // C <= 1024 never asks for more
            const int64_t blocks = (a.n_items * LANES + kBlock - 1) / kBlock;
            if (blocks == 0) return;
            set_kernel("bot::appnp_step_kernel<%d,%d,%d,%s,%s>", VEC, LANES, NCHUNK, EW ? "ew" : "-", DROP ? "drop" : "-");
            hipLaunchKernelGGL((appnp_step_kernel<VEC, LANES, NCHUNK, EW, DROP>), dim3((unsigned)blocks), dim3(kBlock), 0, st, a);
        }
    }
    template <int VEC>
    void wide(int L) const {
        if (L <= 128) run<VEC, 64, 2>();
        else if (L <= 256) run<VEC, 64, 4>();
        else if (L <= 512) run<VEC, 64, 8>();
        else run<VEC, 64, 16>();
    }
};

}  // namespace bot

extern "C" {

int bot_appnp_step_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                       const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, const float* y, int64_t ldy, const float* y0,
                       int64_t ldy0, float* out, int64_t ldo, int32_t C, float a, float b, const float* src_scale, const float* dst_scale,
                       const float* out_scale, const float* acc_in, int64_t ldai, float* acc_out, int64_t ldao, float* partial,
                       const float* ew, const int32_t* pos, float p, uint64_t seed, int32_t step, bot_stream_t stream) {
    using namespace bot;
    (void)indptr;
    if (int rc = check_plan_sizes("appnp_step", n_rows, nnz, n_items, n_long)) return rc;
    BOT_REQUIRE(C >= 1 && C <= 1024, BOT_E_RANGE, "appnp_step: C=%d (1..1024)", C);
    BOT_REQUIRE(p >= 0.f && p < 1.f, BOT_E_RANGE, "appnp_step: p=%g (0 <= p < 1)", (double)p);  // a NaN fails both
    BOT_REQUIRE(step >= 0, BOT_E_RANGE, "appnp_step: step=%d is negative", step);
    if (n_rows == 0) return 0;
    if (int rc = check_plan("appnp_step", items, "items/y/out", y && out, nnz, "indices", indices, n_long, "long_rows/long_ptr/partial",
                            long_rows && long_ptr && partial))
        return rc;
    BOT_REQUIRE(acc_out == nullptr || acc_in != nullptr, BOT_E_NULL, "appnp_step: acc_out without acc_in");
    BOT_REQUIRE(out != y, BOT_E_RANGE, "appnp_step: out aliases y (every row of y is read by other rows' sums: use two buffers)");
    BOT_REQUIRE(acc_out == nullptr || acc_out != y, BOT_E_RANGE, "appnp_step: acc_out aliases y (other rows' sums read y while acc_out is written)");
    BOT_REQUIRE(ldy >= C && ldo >= C && (!y0 || ldy0 >= C) && (!acc_out || (ldai >= C && ldao >= C)), BOT_E_RANGE,
                "appnp_step: row strides smaller than C=%d (ldy=%lld ldy0=%lld ldo=%lld ld_acc_in=%lld ld_acc_out=%lld)", C, (long long)ldy,
                (long long)ldy0, (long long)ldo, (long long)ldai, (long long)ldao);
    BOT_REQUIRE(aligned(y, 4) && aligned(y0, 4) && aligned(out, 4) && aligned(acc_in, 4) && aligned(acc_out, 4) && aligned(items, 16) &&
                    aligned(ew, 4) && aligned(pos, 4) && aligned(src_scale, 4) && aligned(dst_scale, 4) && aligned(out_scale, 4) &&
                    aligned(partial, 4),
                BOT_E_ALIGN, "appnp_step: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    if (!acc_out) acc_in = nullptr, ldai = ldao = C;  // not read without a destination
    if (!y0) ldy0 = C;
    const AppnpArgs g{indices, reinterpret_cast<const int4*>(items), n_items, y, ldy, y0, ldy0, out, ldo, C, a, b, src_scale, dst_scale,
                      out_scale, acc_in, ldai, acc_out, ldao, partial, ew, pos, p, 1.0f / (1.0f - p), seed, (uint32_t)step};
    const int vec = pick_vec(C, {ldy, ldy0, ldo, ldai, ldao}, {y, y0, out, acc_in, acc_out, partial});
    const bool drop = p > 0.f;
    if (ew && drop) dispatch_sweep(AppnpLaunch<true, true>{g, st}, C, vec);
    else if (ew) dispatch_sweep(AppnpLaunch<true, false>{g, st}, C, vec);
    else if (drop) dispatch_sweep(AppnpLaunch<false, true>{g, st}, C, vec);
    else dispatch_sweep(AppnpLaunch<false, false>{g, st}, C, vec);
    if (int rc = hip_status("appnp_step launch")) return rc;
    if (n_long > 0) {
        hipLaunchKernelGGL(appnp_combine_kernel, dim3((unsigned)((n_long * 64 + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, g, long_rows, long_ptr,
                           n_long);
        if (int rc = hip_status("appnp_step combine launch")) return rc;
    }
    return 0;
}

}  // extern "C"
