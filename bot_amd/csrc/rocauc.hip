// Exact multi-task ROC-AUC counts (OGB's "rocauc": the Mann-Whitney statistic per task), gfx950.  include/bot_gnn.h bot_rocauc_f32.
//
// For every (group g, task t): n_pos, n_neg and 2U = sum over (positive p, negative q) pairs of the group of 2 [s_q < s_p] + [s_q == s_p],
// all int64 - integer arithmetic and integer atomics only, so the result is a pure function of the inputs.
//
//   prep        pred [n, T] -> task-major order-preserving uint32 keys (-0.0 folded onto +0.0, then sign flip) and one code byte per
//               entry ((g << 1) | label, 0xFF = not counted), through a 64 x 64 LDS transpose; NaNs of counted entries are counted.
//   4 x (tile_hist, scan, scatter)   least-significant-digit radix sort of (key, code) per task, 8 bits per pass; grid = (tiles, tasks):
//               the stable passes of radix.h, shared with the graph builder (plan.hip).
//   tile_count, tile_prefix   negatives per (task, 2048-entry tile, group), prefix over the tiles; n_pos / n_neg into the output.
//   sweep       2U = sum over positives p of N(start of p's tie run) + N(end of p's tie run), N(x) = the group's negatives in sorted
//               positions [0, x).  Runs inside a tile are located by binary search in LDS; the run a tile starts or ends in is
//               followed across tiles by binary search in the sorted column, its N by the tile prefix plus one partial tile.
//
// Every global index is t * n + i < 2^40 (int64); positions inside a task are uint32 (n < 2^31).
#include "common.h"
#include "radix.h"

namespace bot {

constexpr int kRocTile = kRadixTile;                              // sort tile (radix.h): 4096 entries
constexpr int kRocSweepItems = 8, kRocSweep = kBlock * kRocSweepItems;   // sweep tile: 2048 entries (16-bit packed counts hold it)
constexpr uint8_t kRocSkip = 0xFF;

struct RocWorkspace {
    int64_t keys_a, keys_b, codes_a, codes_b, hist, negs, total;   // byte offsets
    int64_t tiles, sweep_tiles;
};

static inline int64_t roc_align(int64_t x) { return (x + 255) / 256 * 256; }

static RocWorkspace roc_workspace(int64_t n, int64_t T) {
    RocWorkspace w;
    w.tiles = (n + kRocTile - 1) / kRocTile;
    w.sweep_tiles = (n + kRocSweep - 1) / kRocSweep;
    int64_t o = 0;
    w.keys_a = o, o += roc_align(n * T * 4);
    w.keys_b = o, o += roc_align(n * T * 4);
    w.codes_a = o, o += roc_align(n * T);
    w.codes_b = o, o += roc_align(n * T);
    w.hist = o, o += roc_align(T * w.tiles * 256 * 4);
    w.negs = o, o += roc_align(T * (w.sweep_tiles + 1) * 8 * 4);
    w.total = o;
    return w;
}

__global__ __launch_bounds__(kBlock) void rocauc_zero_kernel(int64_t* __restrict__ out, int64_t m, int64_t* __restrict__ nan_count) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i < m) out[i] = 0;
    if (i == 0) *nan_count = 0;
}

__global__ __launch_bounds__(kBlock) void rocauc_prep_kernel(const float* __restrict__ pred, int64_t ldp, const int8_t* __restrict__ labels, int64_t ldl,
                                                             const int8_t* __restrict__ groups, int64_t n, int32_t T, int32_t G,
                                                             uint32_t* __restrict__ keys, uint8_t* __restrict__ codes,
                                                             unsigned long long* __restrict__ nan_count) {
    __shared__ uint32_t sk[64][65];
    __shared__ uint8_t sc[64][65];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t i0 = (int64_t)blockIdx.x * 64;
    const int32_t t0 = (int32_t)blockIdx.y * 64;
    uint32_t nans = 0;
    for (int r = ty; r < 64; r += 4) {
        const int64_t i = i0 + r;
        const int32_t t = t0 + tx;
        uint32_t key = 0xFFFFFFFFu;
        uint8_t code = kRocSkip;
        if (i < n && t < T) {
            uint32_t b = __float_as_uint(pred[i * ldp + t]);
            const int g = groups ? (int)groups[i] : 0;
            const int l = (int)labels[i * ldl + t];
            const bool counted = g >= 0 && g < G && (l == 0 || l == 1);
            const bool is_nan = (b & 0x7FFFFFFFu) > 0x7F800000u;
            if (counted && is_nan) ++nans;
            if (counted && !is_nan) code = (uint8_t)((g << 1) | l);
            if (b == 0x80000000u) b = 0u;                                   // -0.0 == +0.0
            key = (b & 0x80000000u) ? ~b : (b | 0x80000000u);               // unsigned order == IEEE order (denormals kept apart)
        }
        sk[r][tx] = key;
        sc[r][tx] = code;
    }
    __syncthreads();
    for (int c = ty; c < 64; c += 4) {
        const int64_t i = i0 + tx;
        const int32_t t = t0 + c;
        if (i < n && t < T) {
            keys[(int64_t)t * n + i] = sk[tx][c];
            codes[(int64_t)t * n + i] = sc[tx][c];
        }
    }
    if (nans) atomicAdd(nan_count, (unsigned long long)nans);
}

// packed counts: group g's count sits in bits 16 (g & 3) .. of word g >> 2 (a 2048-entry tile: below 2^16 each)
struct Pack2 {
    unsigned long long a, b;
};
__device__ __forceinline__ Pack2 roc_pack_neg(uint8_t code) {
    Pack2 p{0ull, 0ull};
    if (code != kRocSkip && !(code & 1)) {
        const int g = code >> 1;
        const unsigned long long one = 1ull << (16 * (g & 3));
        if (g < 4) p.a = one;
        else p.b = one;
    }
    return p;
}
__device__ __forceinline__ uint32_t roc_unpack(unsigned long long a, unsigned long long b, int g) {
    return (uint32_t)(((g < 4 ? a : b) >> (16 * (g & 3))) & 0xFFFFull);
}

// negs[(t * (sweep_tiles + 1) + tile) * 8 + g] = negatives of group g in the tile; out[(g T + t) 3 + {0, 1}] += the tile's positives / negatives
__global__ __launch_bounds__(kBlock) void rocauc_tile_count_kernel(const uint8_t* __restrict__ codes, int64_t n, int32_t T, int32_t G,
                                                                   uint32_t* __restrict__ negs, unsigned long long* __restrict__ out) {
    __shared__ uint32_t cnt[16];
    if (threadIdx.x < 16) cnt[threadIdx.x] = 0;
    __syncthreads();
    const int64_t t = blockIdx.y, start = (int64_t)blockIdx.x * kRocSweep;
    const uint8_t* c = codes + t * n;
#pragma unroll
    for (int e = 0; e < kRocSweepItems; ++e) {
        const int64_t i = start + e * kBlock + threadIdx.x;
        if (i < n) {
            const uint8_t code = c[i];
            if (code != kRocSkip) atomicAdd(&cnt[code & 15], 1u);
        }
    }
    __syncthreads();
    if (threadIdx.x < 8) negs[(t * (gridDim.x + 1) + blockIdx.x) * 8 + threadIdx.x] = cnt[2 * threadIdx.x];
    if (threadIdx.x < 2 * G && cnt[threadIdx.x]) {
        const int g = threadIdx.x >> 1, pos = threadIdx.x & 1;
        atomicAdd(&out[((int64_t)g * T + t) * 3 + (pos ? 0 : 1)], (unsigned long long)cnt[threadIdx.x]);
    }
}

// per task and group: exclusive prefix over the tiles; entry [sweep_tiles] = the total
__global__ __launch_bounds__(kWave) void rocauc_tile_prefix_kernel(uint32_t* __restrict__ negs, int64_t sweep_tiles) {
    if (threadIdx.x >= 8) return;
    uint32_t* p = negs + (int64_t)blockIdx.x * (sweep_tiles + 1) * 8 + threadIdx.x;
    uint32_t run = 0;
    for (int64_t k = 0; k < sweep_tiles; ++k) {
        const uint32_t v = p[k * 8];
        p[k * 8] = run;
        run += v;
    }
    p[sweep_tiles * 8] = run;
}

__global__ __launch_bounds__(kBlock) void rocauc_sweep_kernel(const uint32_t* __restrict__ keys, const uint8_t* __restrict__ codes, int64_t n, int32_t T,
                                                              int32_t G, const uint32_t* __restrict__ negs, unsigned long long* __restrict__ out) {
    __shared__ uint32_t sk[kRocSweep];
    __shared__ uint8_t sc[kRocSweep];
    __shared__ unsigned long long pa[kRocSweep + 1], pb[kRocSweep + 1];   // packed negatives in [0, j) of the tile
    __shared__ unsigned long long wave_a[4], wave_b[4], part[2], acc[8];
    __shared__ int64_t bound[2];
    __shared__ uint32_t n_start[8], n_end[8], base[8];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t t = blockIdx.y, tile = blockIdx.x, sweep_tiles = gridDim.x, start = tile * kRocSweep;
    const int len = (int)((n - start) < kRocSweep ? (n - start) : kRocSweep);
    const uint32_t* k = keys + t * n;
    const uint8_t* c = codes + t * n;
    const uint32_t* tn = negs + t * (sweep_tiles + 1) * 8;
#pragma unroll
    for (int e = 0; e < kRocSweepItems; ++e) {
        const int j = e * kBlock + tid;
        sk[j] = j < len ? k[start + j] : 0xFFFFFFFFu;
        sc[j] = j < len ? c[start + j] : kRocSkip;
    }
    if (tid < 8) acc[tid] = 0, base[tid] = tn[tile * 8 + tid];
    if (tid < 2) part[tid] = 0;
    __syncthreads();
    // exclusive packed prefix: thread tid owns entries 8 tid .. 8 tid + 7
    Pack2 loc[kRocSweepItems], sum{0ull, 0ull};
#pragma unroll
    for (int e = 0; e < kRocSweepItems; ++e) {
        loc[e] = sum;
        const Pack2 v = roc_pack_neg(sc[tid * kRocSweepItems + e]);
        sum.a += v.a, sum.b += v.b;
    }
    Pack2 inc = sum;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long ua = __shfl_up(inc.a, o), ub = __shfl_up(inc.b, o);
        if (lane >= o) inc.a += ua, inc.b += ub;
    }
    if (lane == 63) wave_a[w] = inc.a, wave_b[w] = inc.b;
    __syncthreads();
    Pack2 before{inc.a - sum.a, inc.b - sum.b};
    for (int v = 0; v < w; ++v) before.a += wave_a[v], before.b += wave_b[v];
#pragma unroll
    for (int e = 0; e < kRocSweepItems; ++e) {
        pa[tid * kRocSweepItems + e] = before.a + loc[e].a;
        pb[tid * kRocSweepItems + e] = before.b + loc[e].b;
    }
    if (tid == kBlock - 1) pa[kRocSweep] = before.a + sum.a, pb[kRocSweep] = before.b + sum.b;
    // the run the tile starts in begins at bound[0]; the run it ends in stops before bound[1]  (sorted column, binary search)
    if (tid == 0) {
        const uint32_t kf = sk[0];
        int64_t lo = 0, hi = start;                       // first position whose key is not below kf
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (k[mid] < kf) lo = mid + 1;
            else hi = mid;
        }
        bound[0] = lo;
    }
    if (tid == 64) {
        const uint32_t kl = sk[len - 1];
        int64_t lo = start + len, hi = n;                 // first position whose key is above kl
        while (lo < hi) {
            const int64_t mid = lo + (hi - lo) / 2;
            if (k[mid] <= kl) lo = mid + 1;
            else hi = mid;
        }
        bound[1] = lo;
    }
    __syncthreads();
    // N(bound) per group: the tile prefix of the bound's tile + the entries of that tile in front of the bound
    for (int side = 0; side < 2; ++side) {
        const int64_t x = bound[side];
        const bool local = side == 0 ? x == start : x == start + len;
        if (local) {
            if (tid < 8) (side == 0 ? n_start : n_end)[tid] = base[tid] + (side == 0 ? 0u : roc_unpack(pa[len], pb[len], tid));
        } else {
            const int64_t xt = x / kRocSweep, x0 = xt * kRocSweep;
            Pack2 s{0ull, 0ull};
            for (int64_t i = x0 + tid; i < x; i += kBlock) {
                const Pack2 v = roc_pack_neg(c[i]);
                s.a += v.a, s.b += v.b;
            }
            if (s.a) atomicAdd(&part[0], s.a);
            if (s.b) atomicAdd(&part[1], s.b);
            __syncthreads();
            if (tid < 8) (side == 0 ? n_start : n_end)[tid] = tn[xt * 8 + tid] + roc_unpack(part[0], part[1], tid);
            __syncthreads();
            if (tid < 2) part[tid] = 0;
        }
        __syncthreads();
    }
    const uint32_t kf = sk[0], kl = sk[len - 1];
    unsigned long long mine[8] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
#pragma unroll
    for (int e = 0; e < kRocSweepItems; ++e) {
        const int j = e * kBlock + tid;
        const uint8_t code = sc[j];
        if (j < len && code != kRocSkip && (code & 1)) {
            const int g = code >> 1;
            const uint32_t key = sk[j];
            uint32_t below, through;
            if (key == kf) below = n_start[g];
            else {
                int lo = 0, hi = j;                       // first entry of the tile with this key
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (sk[mid] < key) lo = mid + 1;
                    else hi = mid;
                }
                below = base[g] + roc_unpack(pa[lo], pb[lo], g);
            }
            if (key == kl) through = n_end[g];
            else {
                int lo = j + 1, hi = len;                 // first entry of the tile above this key
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (sk[mid] <= key) lo = mid + 1;
                    else hi = mid;
                }
                through = base[g] + roc_unpack(pa[lo], pb[lo], g);
            }
            const unsigned long long v = (unsigned long long)below + through;
#pragma unroll
            for (int q = 0; q < 8; ++q) mine[q] += q == g ? v : 0ull;
        }
    }
#pragma unroll
    for (int q = 0; q < 8; ++q)
        if (mine[q]) atomicAdd(&acc[q], mine[q]);
    __syncthreads();
    if (tid < G && acc[tid]) atomicAdd(&out[((int64_t)tid * T + t) * 3 + 2], acc[tid]);
}

}  // namespace bot

extern "C" int64_t bot_rocauc_workspace_bytes(int64_t n, int32_t T, int32_t G) {
    if (n < 0 || n >= (1ll << 31) || T < 1 || T > 65535 || G < 1 || G > 8 || n * (int64_t)T >= (1ll << 40)) return -1;
    return bot::roc_workspace(n, T).total;
}

extern "C" int bot_rocauc_f32(const float* pred, int64_t ldp, const int8_t* labels, int64_t ldl, const int8_t* groups, int64_t n, int32_t T, int32_t G,
                              int64_t* out, int64_t* nan_count, void* workspace, int64_t workspace_bytes, bot_stream_t stream) {
    using namespace bot;
    BOT_REQUIRE(n >= 0 && n < (1ll << 31) && T >= 1 && T <= 65535 && G >= 1 && G <= 8 && n * (int64_t)T < (1ll << 40) && ldp >= T && ldl >= T,
                BOT_E_RANGE, "rocauc: n=%lld T=%d G=%d ldp=%lld ldl=%lld (0 <= n < 2^31, 1 <= T <= 65535, 1 <= G <= 8, n T < 2^40, ld >= T)",
                (long long)n, (int)T, (int)G, (long long)ldp, (long long)ldl);
    BOT_REQUIRE(out != nullptr && nan_count != nullptr, BOT_E_NULL, "rocauc: out / nan_count is NULL");
    if (n == 0) return 0;                                  // nothing is launched: the caller's zeros stay
    const RocWorkspace ws = roc_workspace(n, T);
    BOT_REQUIRE(pred != nullptr && labels != nullptr && workspace != nullptr, BOT_E_NULL, "rocauc: pred / labels / workspace is NULL");
    BOT_REQUIRE(workspace_bytes >= ws.total, BOT_E_RANGE, "rocauc: workspace of %lld bytes, bot_rocauc_workspace_bytes asks for %lld",
                (long long)workspace_bytes, (long long)ws.total);
    BOT_REQUIRE(aligned(workspace, 8), BOT_E_ALIGN, "rocauc: workspace is not 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    char* base = (char*)workspace;
    uint32_t *ka = (uint32_t*)(base + ws.keys_a), *kb = (uint32_t*)(base + ws.keys_b), *hist = (uint32_t*)(base + ws.hist),
             *negs = (uint32_t*)(base + ws.negs);
    uint8_t *ca = (uint8_t*)(base + ws.codes_a), *cb = (uint8_t*)(base + ws.codes_b);
    unsigned long long* uout = (unsigned long long*)out;
    const int64_t m = (int64_t)G * T * 3;
    set_kernel("radix_scatter_kernel");
    hipLaunchKernelGGL(rocauc_zero_kernel, dim3((unsigned)((m + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, out, m, nan_count);
    hipLaunchKernelGGL(rocauc_prep_kernel, dim3((unsigned)((n + 63) / 64), (unsigned)((T + 63) / 64)), dim3(kBlock), 0, st, pred, ldp, labels, ldl, groups,
                       n, T, G, ka, ca, (unsigned long long*)nan_count);
    for (int pass = 0; pass < 4; ++pass) {
        const int32_t shift = 8 * pass;
        radix_pass<uint8_t>(ka, ca, n, T, shift, hist, kb, cb, st);
        uint32_t* tk = ka;
        ka = kb, kb = tk;
        uint8_t* tc = ca;
        ca = cb, cb = tc;
    }
    const dim3 sgrid((unsigned)ws.sweep_tiles, (unsigned)T);
    hipLaunchKernelGGL(rocauc_tile_count_kernel, sgrid, dim3(kBlock), 0, st, ca, n, T, G, negs, uout);
    hipLaunchKernelGGL(rocauc_tile_prefix_kernel, dim3((unsigned)T), dim3(kWave), 0, st, negs, ws.sweep_tiles);
    hipLaunchKernelGGL(rocauc_sweep_kernel, sgrid, dim3(kBlock), 0, st, ka, ca, n, T, G, negs, uout);
    return hip_status("rocauc launch");
}
