// One sweep of label propagation / Correct and Smooth (include/bot_gnn.h "Propagation step") for gfx950:
//   out[v,:] = fixed[v] ? y0[v,:] : clamp(alpha * dst_scale[v] * sum_k src_scale[indices[k]] * y[indices[k],:] + beta * y0[v,:], lo, hi)
//   row_abs[v] = sum_c |out[v,c]|;  with out_scale the row is STORED as out_scale[v] * out[v,:]
//
// The gather is the lane-group row sweep that sweep.h describes; src_scale[id] is read beside the ids and broadcast with them.  What differs from the
// SpMM is everything behind the sum: the row scale, the axpy with the start matrix, the clamp, the reset of fixed rows and the row's L1
// norm are the epilogue of the lane group that owns the row, so an iteration is one launch and [N, C] is read and written once.  The
// chunks of a long row leave their raw sums in `partial`; prop_combine_kernel adds them in slot order and runs the same epilogue.
// Plain stores only: no atomics, the bytes repeat from call to call.
//
// src_scale[id] is a second random read per edge, into a table of N floats.  S-arxiv's 0.7 MB stay in the L2; S-products' 9.8 MB do
// not, and a sweep took 6.5 ms against 5.0 ms of the SpMM with streamed edge weights.  So out_scale stores the row already
// multiplied by the NEXT sweep's source scale: that sweep passes src_scale = NULL and gathers rows only (bot_amd/smoothing.py
// runs every sweep but the first one that way).
//
// HBM model per sweep: 4 * [E * (1 + 1 + C) + 3 * N * C] bytes (ids, source scales and source rows per edge; y0, out and the
// gathered table per node); a pre-scaled sweep drops one of the two words per edge.
//
// Edge weights (bot_propagate_step_w_f32, the EW instances): ew[k], float32 in CSC position order, is read by the lane that reads
// indices[k] - two sequential loads that leave together, no load level in front of the row gathers - and multiplied into that
// lane's source scale before the broadcast (sv *= ew[k]), so a weight of 1.0f leaves every product and every byte as it is.  The
// chunks of a long row take their weights the same way; prop_combine_kernel and the epilogue see sums only.  out_scale is a per-node
// factor and works as before.  HBM model per sweep: one more streamed 4-byte word per edge, 4 * [E * (1 + 1 + 1 + C) + 3 * N * C]
// bytes (a pre-scaled sweep: E * (1 + 1 + C)).  The instances without EW are the code they were.
#include "sweep.h"

#include <initializer_list>

namespace bot {

struct PropArgs {
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
    float alpha, beta;
    const float* src_scale;
    const float* dst_scale;
    float lo, hi;
    const uint8_t* fixed;
    float* row_abs;
    const float* out_scale;
    float* partial;
    const float* ew;
};

// The epilogue of VEC consecutive columns of row `row`: s holds the gathered sums on entry and the stored values on return; returns
// the absolute sum of the row's values before `osc`, the factor they are stored with.  The clamp is written with comparisons so that a
// NaN stays a NaN (torch.clamp's rule).
template <int VEC>
__device__ __forceinline__ float prop_finish(const PropArgs& a, int row, int col, float av, bool fx, float osc, float (&s)[VEC]) {
    float r[VEC], ra = 0.f;
    vload<VEC>(r, a.y0 + (int64_t)row * a.ldy0 + col);
#pragma unroll
    for (int t = 0; t < VEC; ++t) {
        float o = fmaf(av, s[t], a.beta * r[t]);
        o = o < a.lo ? a.lo : o;
        o = o > a.hi ? a.hi : o;
        o = fx ? r[t] : o;
        ra += fabsf(o);
        s[t] = o * osc;
    }
    vstore<VEC>(a.out + (int64_t)row * a.ldo + col, s);
    return ra;
}

template <int VEC, int LANES, int NCHUNK, bool EW = false>
__global__ __launch_bounds__(kBlock) void prop_step_kernel(PropArgs a) {
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
            if (a.src_scale) sv = a.src_scale[idx];
            if constexpr (EW) sv *= wk;
        }
        const int cnt = min(LANES, it.end - k0);
        int i = 0;
        for (; i + U <= cnt; i += U) {
            float v[U][NCHUNK][VEC], ww[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int s = group_bcast<LANES>(idx, i + u);
                ww[u] = group_bcast<LANES>(sv, i + u);
                const float* p = a.y + (int64_t)s * a.ldy;
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c) vload<VEC>(v[u][c], p + tile.off[c]);
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
    if (it.slot >= 0) {  // a chunk of a long row: the raw sum, finished by prop_combine_kernel
        tile.store(a.partial + (int64_t)it.slot * a.C, acc);
        return;
    }
    const float av = a.alpha * (a.dst_scale ? a.dst_scale[row] : 1.f);
    const bool fx = a.fixed && a.fixed[row] != 0;
    const float osc = a.out_scale ? a.out_scale[row] : 1.f;
    float ra = 0.f;
#pragma unroll
    for (int c = 0; c < NCHUNK; ++c)
        if (tile.act[c]) ra += prop_finish<VEC>(a, row, tile.off[c], av, fx, osc, acc[c]);
    if (a.row_abs) {  // the whole group is here (slot is uniform over it): lanes in column order, then the butterfly
        ra = group_sum<LANES>(ra);
        if (lane == 0) a.row_abs[row] = ra;
    }
}

// One wavefront per long row: column c = lane, lane + 64, ...; the chunk sums are added in slot order, then the row's epilogue.
__global__ __launch_bounds__(kBlock) void prop_combine_kernel(PropArgs a, const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long) {
    const int lane = threadIdx.x & 63;
    const int64_t i = ((int64_t)blockIdx.x * kBlock + threadIdx.x) >> 6;
    if (i >= n_long) return;  // whole waves leave together
    const int row = long_rows[i], p0 = long_ptr[i], p1 = long_ptr[i + 1];
    const float av = a.alpha * (a.dst_scale ? a.dst_scale[row] : 1.f);
    const bool fx = a.fixed && a.fixed[row] != 0;
    const float osc = a.out_scale ? a.out_scale[row] : 1.f;
    float ra = 0.f;
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
        ra += prop_finish<1>(a, row, c, av, fx, osc, s);
    }
    if (a.row_abs) {
        ra = group_sum<64>(ra);
        if (lane == 0) a.row_abs[row] = ra;
    }
}

template <bool EW>
struct PropLaunch {
    const PropArgs& a;
    hipStream_t st;
    template <int VEC, int LANES, int NCHUNK>
    void run() const {
        if constexpr (VEC * NCHUNK <= 16) {  // C <= 1024 never asks for more
            const int64_t blocks = (a.n_items * LANES + kBlock - 1) / kBlock;
            if (blocks == 0) return;
            set_kernel(EW ? "bot::prop_step_kernel<%d,%d,%d,ew>" : "bot::prop_step_kernel<%d,%d,%d>", VEC, LANES, NCHUNK);
            hipLaunchKernelGGL((prop_step_kernel<VEC, LANES, NCHUNK, EW>), dim3((unsigned)blocks), dim3(kBlock), 0, st, a);
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

// both entry points; ew == NULL runs the instances without EW
static int propagate_step(const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items, const int32_t* long_rows,
                          const int32_t* long_ptr, int64_t n_long, const float* y, int64_t ldy, const float* y0, int64_t ldy0, float* out,
                          int64_t ldo, int32_t C, float alpha, float beta, const float* src_scale, const float* dst_scale, float lo, float hi,
                          const uint8_t* fixed, float* row_abs, const float* out_scale, float* partial, const float* ew, bot_stream_t stream) {
    if (int rc = check_plan_sizes("propagate_step", n_rows, nnz, n_items, n_long)) return rc;
    BOT_REQUIRE(C >= 1 && C <= 1024, BOT_E_RANGE, "propagate_step: C=%d (1..1024)", C);
    if (n_rows == 0) return 0;
    if (int rc = check_plan("propagate_step", items, "items/y/y0/out", y && y0 && out, nnz, "indices", indices, n_long,
                            "long_rows/long_ptr/partial", long_rows && long_ptr && partial))
        return rc;
    BOT_REQUIRE(out != y, BOT_E_RANGE, "propagate_step: out aliases y (every row of y is read by other rows' sums: use two buffers)");
    BOT_REQUIRE(ldy >= C && ldy0 >= C && ldo >= C, BOT_E_RANGE, "propagate_step: row strides smaller than C=%d (ldy=%lld ldy0=%lld ldo=%lld)", C,
                (long long)ldy, (long long)ldy0, (long long)ldo);
    BOT_REQUIRE(aligned(y, 4) && aligned(y0, 4) && aligned(out, 4) && aligned(items, 16) && aligned(ew, 4), BOT_E_ALIGN,
                "propagate_step: misaligned pointer");
    hipStream_t st = (hipStream_t)stream;
    const PropArgs a{indices, reinterpret_cast<const int4*>(items), n_items, y, ldy, y0, ldy0, out, ldo, C, alpha, beta, src_scale, dst_scale,
                     lo, hi, fixed, row_abs, out_scale, partial, ew};
    const int vec = pick_vec(C, {ldy, ldy0, ldo}, {y, y0, out, partial});
    if (ew) dispatch_sweep(PropLaunch<true>{a, st}, C, vec);
    else dispatch_sweep(PropLaunch<false>{a, st}, C, vec);
    if (int rc = hip_status("propagate_step launch")) return rc;
    if (n_long > 0) {
        hipLaunchKernelGGL(prop_combine_kernel, dim3((unsigned)((n_long * 64 + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, a, long_rows, long_ptr,
                           n_long);
        if (int rc = hip_status("propagate_step combine launch")) return rc;
    }
    return 0;
}

}  // namespace bot

extern "C" {

int bot_propagate_step_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                           const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, const float* y, int64_t ldy, const float* y0,
                           int64_t ldy0, float* out, int64_t ldo, int32_t C, float alpha, float beta, const float* src_scale,
                           const float* dst_scale, float lo, float hi, const uint8_t* fixed, float* row_abs, const float* out_scale,
                           float* partial, bot_stream_t stream) {
    (void)indptr;
    return bot::propagate_step(indices, n_rows, nnz, items, n_items, long_rows, long_ptr, n_long, y, ldy, y0, ldy0, out, ldo, C, alpha, beta,
                               src_scale, dst_scale, lo, hi, fixed, row_abs, out_scale, partial, nullptr, stream);
}

int bot_propagate_step_w_f32(const int32_t* indptr, const int32_t* indices, int64_t n_rows, int64_t nnz, const int32_t* items, int64_t n_items,
                             const int32_t* long_rows, const int32_t* long_ptr, int64_t n_long, const float* y, int64_t ldy, const float* y0,
                             int64_t ldy0, float* out, int64_t ldo, int32_t C, float alpha, float beta, const float* src_scale,
                             const float* dst_scale, float lo, float hi, const uint8_t* fixed, float* row_abs, const float* out_scale,
                             float* partial, const float* ew, bot_stream_t stream) {
    (void)indptr;
    return bot::propagate_step(indices, n_rows, nnz, items, n_items, long_rows, long_ptr, n_long, y, ldy, y0, ldy0, out, ldo, C, alpha, beta,
                               src_scale, dst_scale, lo, hi, fixed, row_abs, out_scale, partial, ew, stream);
}

}  // extern "C"
