// One pass of a stable least-significant-digit radix sort of (uint32 key, payload) pairs, 8 bits per pass: tile histogram -> scan ->
// stable scatter.  Shared by the ROC-AUC sort (rocauc.hip: payload = one code byte, one sort per task) and the graph builder (plan.hip:
// payload = a row id or a CSC position).  Integer arithmetic and LDS integer atomics only; no atomic decides a position, so the output is
// a pure function of the input.  No kernel waits for another workgroup: the three steps are three launches.
//
//   grid = (tiles, tasks); task t sorts keys[t * n .. t * n + n).  A tile is 4096 consecutive entries.
//   hist[(t * tiles + tile) * 256 + d]: after radix_tile_hist_kernel the tile's count of digit d, after radix_scan_kernel the position in
//   the task's sorted run where the tile's first entry of digit d lands.
//   The scatter is stable: wave w owns a contiguous quarter of the tile, the rank inside a round of 64 comes from __ballot matches, the
//   rounds before it from a per-wave running count in LDS.
#pragma once
#include "common.h"

namespace bot {

constexpr int kRadixItems = 16, kRadixTile = kBlock * kRadixItems;      // sort tile: 4096 entries

inline int64_t radix_tiles(int64_t n) { return (n + kRadixTile - 1) / kRadixTile; }

// hist[(t * tiles + tile) * 256 + d] = entries of the tile whose digit (key >> shift) & 255 is d
static __global__ __launch_bounds__(kBlock) void radix_tile_hist_kernel(const uint32_t* __restrict__ keys, int64_t n, int32_t shift,
                                                                        uint32_t* __restrict__ hist) {
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t t = blockIdx.y, start = (int64_t)blockIdx.x * kRadixTile;
    const uint32_t* k = keys + t * n;
#pragma unroll
    for (int e = 0; e < kRadixItems; ++e) {
        const int64_t i = start + e * kBlock + threadIdx.x;
        if (i < n) atomicAdd(&h[(k[i] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(t * gridDim.x + blockIdx.x) * 256 + threadIdx.x] = h[threadIdx.x];
}

// per task: hist[tile][d] -> the position in the task's sorted run where the tile's first entry of digit d lands
static __global__ __launch_bounds__(kBlock) void radix_scan_kernel(uint32_t* __restrict__ hist, int64_t tiles) {
    __shared__ uint32_t tot[256];
    uint32_t* h = hist + (int64_t)blockIdx.x * tiles * 256;
    const int d = threadIdx.x;
    uint32_t sum = 0;
    for (int64_t k = 0; k < tiles; ++k) sum += h[k * 256 + d];
    tot[d] = sum;
    __syncthreads();
    if (d == 0) {
        uint32_t run = 0;
        for (int j = 0; j < 256; ++j) {
            const uint32_t v = tot[j];
            tot[j] = run;
            run += v;
        }
    }
    __syncthreads();
    uint32_t run = tot[d];
    for (int64_t k = 0; k < tiles; ++k) {
        const uint32_t v = h[k * 256 + d];
        h[k * 256 + d] = run;
        run += v;
    }
}

template <typename P>
__global__ __launch_bounds__(kBlock) void radix_scatter_kernel(const uint32_t* __restrict__ keys_in, const P* __restrict__ vals_in, int64_t n,
                                                               int32_t shift, const uint32_t* __restrict__ hist, uint32_t* __restrict__ keys_out,
                                                               P* __restrict__ vals_out) {
    __shared__ uint32_t run[4][256];       // per wave: where the wave's next entry of digit d goes
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t t = blockIdx.y, start = (int64_t)blockIdx.x * kRadixTile + (int64_t)w * (kRadixItems * 64);
    const uint32_t* k = keys_in + t * n;
    const P* c = vals_in + t * n;
    for (int j = lane; j < 256; j += 64) run[w][j] = 0;
    __syncthreads();
    uint32_t key[kRadixItems];
    P val[kRadixItems];
#pragma unroll
    for (int e = 0; e < kRadixItems; ++e) {
        const int64_t i = start + e * 64 + lane;
        const bool ok = i < n;
        key[e] = ok ? k[i] : 0xFFFFFFFFu;
        val[e] = ok ? c[i] : P{};
        if (ok) atomicAdd(&run[w][(key[e] >> shift) & 255u], 1u);
    }
    __syncthreads();
    {   // counts per wave -> first position per wave: the tile's base + the waves before
        const int d = threadIdx.x;
        uint32_t base = hist[(t * gridDim.x + blockIdx.x) * 256 + d];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const uint32_t cnt = run[v][d];
            run[v][d] = base;
            base += cnt;
        }
    }
    __syncthreads();
    volatile uint32_t* mine = run[w];
    const uint64_t below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
#pragma unroll
    for (int e = 0; e < kRadixItems; ++e) {
        const int64_t i = start + e * 64 + lane;
        const bool ok = i < n;                       // entries past n are the tail of the last tile: nothing valid comes after them
        const uint32_t d = (key[e] >> shift) & 255u;
        uint64_t same = __ballot(ok);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const bool bit = (d >> b) & 1u;
            const uint64_t m = __ballot(bit);
            same &= bit ? m : ~m;
        }
        const uint32_t first = mine[d];
        const uint32_t pos = first + (uint32_t)__popcll(same & below);
        __builtin_amdgcn_wave_barrier();
        if (ok && (same & below) == 0) mine[d] = first + (uint32_t)__popcll(same);   // the lowest lane of the match group
        __builtin_amdgcn_wave_barrier();
        if (ok && pos < n) {
            keys_out[t * n + pos] = key[e];
            vals_out[t * n + pos] = val[e];
        }
    }
}

// One pass on `st`: (keys_in, vals_in) -> (keys_out, vals_out) ordered by the digit at `shift`, stable.  hist: tasks * radix_tiles(n) * 256 words.
template <typename P>
inline void radix_pass(const uint32_t* keys_in, const P* vals_in, int64_t n, int64_t tasks, int32_t shift, uint32_t* hist, uint32_t* keys_out,
                       P* vals_out, hipStream_t st) {
    const int64_t tiles = radix_tiles(n);
    const dim3 grid((unsigned)tiles, (unsigned)tasks);
    hipLaunchKernelGGL(radix_tile_hist_kernel, grid, dim3(kBlock), 0, st, keys_in, n, shift, hist);
    hipLaunchKernelGGL(radix_scan_kernel, dim3((unsigned)tasks), dim3(kBlock), 0, st, hist, tiles);
    hipLaunchKernelGGL(radix_scatter_kernel<P>, grid, dim3(kBlock), 0, st, keys_in, vals_in, n, shift, hist, keys_out, vals_out);
}

}  // namespace bot
