// Edge-weighted neighbour sampling without replacement (DGL's sample_neighbors(..., prob=w) / MultiLayerNeighborSampler(prob=w)),
// gfx950.  The contract is stated in include/bot_gnn.h and restated in numpy in tests/test_weighted_sampling_host.py.
//
// Preparation (once per weight tensor).  One wavefront per CSC row: the row's largest weight w_max = m * 2^e (m in [0.5, 1))
// fixes the scale, q_i = floor(w_i * 2^(33 - e)) (exact in fp64: a power-of-two scale of an fp32 value, then a truncation), and an
// integer inclusive scan of q over the row gives prefix[base + i] = q_0 + .. + q_i.  q_max lies in [2^32, 2^33), so a row of up to
// 2^31 edges sums below 2^64.  The row's number of positive q goes to n_pos; a negative, NaN or infinite weight sets the error flag.
//
// Sampling.  One wavefront per seed.  A row with at most k positive edges is copied whole (a ballot compaction of the q > 0 edges).
// Otherwise k serial rounds of successive sampling: round m draws t = floor(r * Q_rem / 2^96), r = the 96-bit integer
// (x0 << 64 | x1 << 32 | x2) of Philox4x32-10(seed, v << 32 | m) words x0..x2, Q_rem = the total q of the edges not taken yet, and
// takes the smallest offset i whose untaken prefix C(i) = prefix[i] - (q taken at offsets <= i) exceeds t.  C is non-decreasing,
// so a 64-ary search finds i: each lane probes one offset (a global load of the cached prefix) and corrects it by the taken set,
// kept sorted in LDS with the running sum of its q (a binary search per lane).  The pick is inserted into the sorted set (an
// O(k / 64) shift).  O(k (log_64 deg + k / 64)) per row, independent of deg beyond the log: a hub of 10^5 in-edges needs three
// probe rounds per pick.  Integer arithmetic only: deterministic, and a pure function of (graph, weights, v, k, seed).
#include "common.h"

namespace bot {
namespace {

constexpr int kWeightedMaxK = 1024;             // the uniform sampler's bound
constexpr int kWeightedWaves = kBlock / kWave;

__device__ __forceinline__ uint64_t shfl_up_u64(uint64_t x, int d) {
    const uint32_t lo = __shfl_up((uint32_t)x, d), hi = __shfl_up((uint32_t)(x >> 32), d);
    return ((uint64_t)hi << 32) | lo;
}

__device__ __forceinline__ uint64_t shfl_u64(uint64_t x, int src) {
    const uint32_t lo = __shfl((uint32_t)x, src), hi = __shfl((uint32_t)(x >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}

__global__ __launch_bounds__(kBlock) void weights_prepare_kernel(const int32_t* indptr, const int32_t* eid, int64_t n_rows, const float* w,
                                                                 uint64_t* prefix, int32_t* n_pos, int32_t* bad) {
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int64_t n_waves = (int64_t)gridDim.x * kWeightedWaves;
    for (int64_t r = (int64_t)blockIdx.x * kWeightedWaves + wv; r < n_rows; r += n_waves) {
        const int32_t base = indptr[r], deg = indptr[r + 1] - base;
        // non-negative floats order like their bit patterns: the row maximum as an integer maximum
        uint32_t mx = 0;
        bool invalid = false;
        for (int32_t j = lane; j < deg; j += kWave) {
            const float x = w[eid[base + j]];
            invalid |= !(x >= 0.f) || isinf(x);    // negative, NaN or +-inf (-0 counts as zero)
            mx = max(mx, __float_as_uint(x) & 0x7fffffffu);
        }
        if (__any(invalid) && lane == 0) *bad = 1;  // every writer stores the same value
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mx = max(mx, (uint32_t)__shfl_xor(mx, o));
        // q = floor(w * 2^(33 - e)): a power-of-two scale in fp64 is exact for every finite fp32 w (33 - e in [-95, 181])
        int e = 0;
        if (mx) frexp((double)__uint_as_float(mx), &e);
        const double scale = mx ? ldexp(1.0, 33 - e) : 0.0;
        uint64_t carry = 0;
        int32_t pos = 0;
        for (int32_t j0 = 0; j0 < deg; j0 += kWave) {
            const int32_t j = j0 + lane;
            uint64_t q = 0;
            if (j < deg) {
                const float x = w[eid[base + j]];
                if (x > 0.f && !isinf(x)) q = (uint64_t)((double)x * scale);
            }
            pos += __popcll(__ballot(q != 0));
            uint64_t inc = q;
#pragma unroll
            for (int d = 1; d < kWave; d <<= 1) {
                const uint64_t y = shfl_up_u64(inc, d);
                if (lane >= d) inc += y;
            }
            inc += carry;
            if (j < deg) prefix[base + j] = inc;
            carry = shfl_u64(inc, kWave - 1);
        }
        if (lane == 0) n_pos[r] = pos;
    }
}

__global__ __launch_bounds__(kBlock) void weighted_count_kernel(const int32_t* n_pos, const int32_t* seeds, int64_t n_seeds, int32_t k,
                                                                int32_t* counts) {
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < n_seeds; i += (int64_t)gridDim.x * kBlock) {
        const int32_t np = n_pos[seeds[i]];
        counts[i] = (k < 0 || np <= k) ? np : k;
    }
}

// t = floor(r * Q / 2^96) with r = x0 << 64 | x1 << 32 | x2: (hi64 * Q + floor(x2 * Q / 2^32)) >> 64, exact in 128 bits (< 2^128)
__device__ __forceinline__ uint64_t weighted_draw(uint64_t seed, int32_t v, int32_t m, uint64_t Q) {
    uint32_t x[4];
    Philox::gen(seed, ((uint64_t)(uint32_t)v << 32) | (uint32_t)m, x);
    const uint64_t hi = ((uint64_t)x[0] << 32) | x[1];
    const unsigned __int128 lo = ((unsigned __int128)x[2] * Q) >> 32;
    return (uint64_t)(((unsigned __int128)hi * Q + lo) >> 64);
}

// dynamic LDS: per wave, the running sums (uint64 [k]) of all waves first, then the taken offsets (int32 [k]) of all waves
__global__ __launch_bounds__(kBlock) void weighted_rows_kernel(const int32_t* indptr, const uint64_t* prefix, const int32_t* n_pos,
                                                               const int32_t* seeds, int64_t n_seeds, int32_t k, uint64_t seed,
                                                               const int64_t* offsets, int32_t* out) {
    extern __shared__ uint64_t lds[];
    const int lane = threadIdx.x & (kWave - 1), wv = threadIdx.x / kWave;
    const int kk = k > 0 ? k : 1;
    uint64_t* cs = lds + (int64_t)wv * kk;                                          // cs[j] = sum of q over taken[0..j]
    int32_t* taken = reinterpret_cast<int32_t*>(lds + (int64_t)kWeightedWaves * kk) + (int64_t)wv * kk;   // ascending offsets
    const int64_t n_waves = (int64_t)gridDim.x * kWeightedWaves;
    for (int64_t i = (int64_t)blockIdx.x * kWeightedWaves + wv; i < n_seeds; i += n_waves) {
        const int32_t v = seeds[i];
        const int32_t base = indptr[v], deg = indptr[v + 1] - base, np = n_pos[v];
        const uint64_t* P = prefix + base;
        const int64_t o = offsets[i];
        if (k < 0 || np <= k) {                        // every positive edge, in position order
            int32_t done = 0;
            for (int32_t j0 = 0; j0 < deg && done < np; j0 += kWave) {
                const int32_t j = j0 + lane;
                bool pos = false;
                if (j < deg) pos = P[j] != (j ? P[j - 1] : 0ull);
                const uint64_t mask = __ballot(pos);
                if (pos) out[o + done + __popcll(mask & ((1ull << lane) - 1))] = base + j;
                done += __popcll(mask);
            }
            continue;
        }
        uint64_t Qrem = P[deg - 1];
        for (int32_t m = 0; m < k; ++m) {
            const uint64_t t = weighted_draw(seed, v, m, Qrem);
            // smallest p in [lo, hi) with C(p) > t; invariant: C(hi - 1) > t and (lo == 0 or C(lo - 1) <= t)
            int32_t lo = 0, hi = deg;
            int32_t pick;
            for (;;) {
                const int32_t len = hi - lo;
                const int32_t step = len <= kWave ? 1 : (len + kWave - 1) / kWave;
                const bool valid = lane * step < len;
                const int32_t p = min(lo + (lane + 1) * step - 1, hi - 1);
                bool gt = false;
                if (valid) {
                    int32_t a = 0, n = m;                // c = number of taken offsets <= p
                    while (n > 0) {
                        const int32_t half = n >> 1;
                        if (taken[a + half] <= p) {
                            a += half + 1;
                            n -= half + 1;
                        } else {
                            n = half;
                        }
                    }
                    const uint64_t C = P[p] - (a ? cs[a - 1] : 0ull);
                    gt = C > t;
                }
                int32_t f = __ffsll((unsigned long long)__ballot(gt)) - 1;   // exists: the last valid lane probes hi - 1
                f = f < 0 ? 0 : f;                     // (never taken; keeps every load inside the row regardless)
                if (step == 1) {
                    pick = lo + f;
                    break;
                }
                hi = min(lo + (f + 1) * step, hi);
                lo = lo + f * step;
            }
            const uint64_t q = P[pick] - (pick ? P[pick - 1] : 0ull);
            // insert pick into the sorted taken set: shift the entries above its rank c up by one, top chunk first
            int32_t c = 0;
            for (int32_t j = lane; j < m; j += kWave) c += taken[j] < pick;
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d);
            for (int32_t j0 = c + ((m - c - 1) / kWave) * kWave; m > c && j0 >= c; j0 -= kWave) {
                const int32_t j = j0 + lane;
                int32_t tj = 0;
                uint64_t sj = 0;
                if (j < m) tj = taken[j], sj = cs[j];
                lds_wave_fence();
                if (j < m) taken[j + 1] = tj, cs[j + 1] = sj + q;
                lds_wave_fence();
            }
            if (lane == 0) {
                taken[c] = pick;
                cs[c] = (c ? cs[c - 1] : 0ull) + q;
            }
            lds_wave_fence();
            Qrem -= q;
        }
        for (int32_t j = lane; j < k; j += kWave) out[o + j] = base + taken[j];
        lds_wave_fence();                                   // the next row overwrites the taken set
    }
}

}  // namespace
}  // namespace bot

extern "C" {

int bot_sample_weights_prepare_f32(const int32_t* indptr, const int32_t* eid, int64_t n_rows, int64_t n_edges, const float* w,
                                   uint64_t* prefix, int32_t* n_pos, int32_t* flag, bot_stream_t stream) {
    using namespace bot;
    BOT_REQUIRE(n_rows >= 0 && n_edges >= 0 && n_edges <= INT32_MAX, BOT_E_RANGE, "sample_weights_prepare: n_rows=%lld n_edges=%lld",
                (long long)n_rows, (long long)n_edges);
    BOT_REQUIRE(indptr != nullptr && flag != nullptr, BOT_E_NULL, "sample_weights_prepare: NULL indptr / flag");
    if (n_rows == 0) return 0;
    BOT_REQUIRE(n_pos != nullptr && (n_edges == 0 || (eid != nullptr && w != nullptr && prefix != nullptr)), BOT_E_NULL,
                "sample_weights_prepare: NULL eid / w / prefix / n_pos");
    hipStream_t st = (hipStream_t)stream;
    set_kernel("weights_prepare_kernel");
    if (hipMemsetAsync(flag, 0, sizeof(int32_t), st) != hipSuccess) return hip_status("sample_weights_prepare memset");
    hipLaunchKernelGGL(weights_prepare_kernel, dim3(launch_grid(n_rows, kWeightedWaves, 8192)), dim3(kBlock), 0, st, indptr, eid, n_rows, w, prefix,
                       n_pos, flag);
    int rc = hip_status("sample_weights_prepare launch");
    if (rc) return rc;
    int32_t bad = 0;                                   // the one device->host read of a preparation
    if (hipMemcpyAsync(&bad, flag, sizeof(int32_t), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return hip_status("sample_weights_prepare flag read");
    BOT_REQUIRE(!bad, BOT_E_RANGE, "sample_weights_prepare: a weight is negative, NaN or infinite");
    return 0;
}

int bot_sample_neighbors_weighted_count_i32(const int32_t* n_pos, int64_t n_rows, const int32_t* seeds, int64_t n_seeds, int32_t k,
                                            int32_t* counts, bot_stream_t stream) {
    using namespace bot;
    BOT_REQUIRE(n_rows >= 0 && n_seeds >= 0 && k <= kWeightedMaxK, BOT_E_RANGE,
                "sample_neighbors_weighted_count: n_rows=%lld n_seeds=%lld k=%d (k <= %d)", (long long)n_rows, (long long)n_seeds, (int)k,
                kWeightedMaxK);
    BOT_REQUIRE(n_pos != nullptr, BOT_E_NULL, "sample_neighbors_weighted_count: n_pos is NULL");
    if (n_seeds == 0) return 0;
    BOT_REQUIRE(seeds != nullptr && counts != nullptr, BOT_E_NULL, "sample_neighbors_weighted_count: NULL seeds / counts");
    set_kernel("weighted_count_kernel");
    hipLaunchKernelGGL(weighted_count_kernel, dim3(launch_grid(n_seeds, kBlock, 4096)), dim3(kBlock), 0, (hipStream_t)stream, n_pos, seeds, n_seeds,
                       k, counts);
    return hip_status("sample_neighbors_weighted_count launch");
}

int bot_sample_neighbors_weighted_i32(const int32_t* indptr, const uint64_t* prefix, const int32_t* n_pos, int64_t n_rows, const int32_t* seeds,
                                      int64_t n_seeds, int32_t k, uint64_t seed, const int64_t* offsets, int32_t* out, bot_stream_t stream) {
    using namespace bot;
    BOT_REQUIRE(n_rows >= 0 && n_seeds >= 0 && k <= kWeightedMaxK, BOT_E_RANGE,
                "sample_neighbors_weighted: n_rows=%lld n_seeds=%lld k=%d (k <= %d)", (long long)n_rows, (long long)n_seeds, (int)k,
                kWeightedMaxK);
    BOT_REQUIRE(indptr != nullptr && n_pos != nullptr, BOT_E_NULL, "sample_neighbors_weighted: NULL indptr / n_pos");
    if (n_seeds == 0) return 0;
    BOT_REQUIRE(prefix != nullptr && seeds != nullptr && offsets != nullptr && out != nullptr, BOT_E_NULL,
                "sample_neighbors_weighted: NULL prefix / seeds / offsets / out");
    const int kk = k > 0 ? k : 1;
    const size_t lds = (size_t)kWeightedWaves * kk * (sizeof(uint64_t) + sizeof(int32_t));   // 48 KiB per workgroup at k = 1024
    set_kernel("weighted_rows_kernel");
    hipLaunchKernelGGL(weighted_rows_kernel, dim3(launch_grid(n_seeds, kWeightedWaves, 8192)), dim3(kBlock), lds, (hipStream_t)stream, indptr, prefix,
                       n_pos, seeds, n_seeds, k, seed, offsets, out);
    return hip_status("sample_neighbors_weighted launch");
}

}  // extern "C"
