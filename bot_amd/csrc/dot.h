// What the dot-product attention sweeps of dot_attn.hip, plain and with edge features, share: the arguments every sweep has (DotPlan), a lane's
// columns in a tile of whole heads with the reduction over a head's lanes (HeadTile), the keep bit of a head, the number of neighbour
// rows in flight, and the ladder of instances (DotLaunch).
#pragma once
#include "sweep.h"

// Every product of the sweeps is rounded on its own and every fused multiply-add is written out (smx.h switches contraction off for the
// rest of the including file): the sweeps, their chunks and the combine run the same arithmetic, and the logit is the same float32 in
// the forward and in the backward over the destinations.
#include "smx.h"

namespace bot {

constexpr int kDotMaxChunk = 6;  // the widest tile: 64 lanes x VEC x 6

// What the sweeps share: the direction's ids and row plan, the head layout and the logit scale.
struct DotPlan {
    const int32_t* indices;
    const int4* items;
    int64_t n_items;
    int32_t H, D, HD, hpt;  // hpt: whole heads per tile (DotLaunch::run)
    float scale;
};

template <int LANES>
__device__ __forceinline__ constexpr int dot_log2() {
    return LANES == 64 ? 6 : LANES == 32 ? 5 : LANES == 16 ? 4 : 3;
}

// The columns of one lane in a tile of whole heads [col0, end), and the head of each of its chunks.
template <int VEC, int LANES, int NCHUNK>
struct HeadTile {
    int off[NCHUNK], hid[NCHUNK];
    bool act[NCHUNK], first[NCHUNK];  // first: the slot that holds its head's first column (it stores the per-head words)
    int pos, lastlane;                // one-chunk instances: the lane's place in its head, the head's last lane
    int h0, h1, ld;                   // the tile's heads [h0, h1), lanes per head
    __device__ __forceinline__ HeadTile(int col0, int end, int lane, int D) {
#pragma unroll
        for (int c = 0; c < NCHUNK; ++c) {
            const int e = col0 + (c * LANES + lane) * VEC;
            act[c] = e < end;
            off[c] = act[c] ? e : 0;         // idle lanes re-read column 0: always in bounds, never stored
            hid[c] = act[c] ? e / D : -1;    // ... and belong to no head
            first[c] = act[c] && e == hid[c] * D;
        }
        ld = D / VEC;
        h0 = col0 / D;
        h1 = end / D;
        const int fl = hid[0] >= 0 ? (hid[0] * D - col0) / VEC : lane;
        pos = lane - fl;
        lastlane = hid[0] >= 0 ? fl + ld - 1 : lane;
    }
    __device__ __forceinline__ int head(int c) const { return hid[c] < 0 ? 0 : hid[c]; }
    // p[n][c]: the lane's partial sums of N quantities -> the totals over the head of chunk c, on every lane of that head
    template <int N>
    __device__ __forceinline__ void total(float (&p)[N][NCHUNK]) const {
        if constexpr (NCHUNK == 1) {
#pragma unroll
            for (int s = 0; s < dot_log2<LANES>(); ++s)
                if ((1 << s) < ld) {  // (uniform) steps at least a head long join nothing
#pragma unroll
                    for (int n = 0; n < N; ++n) {
                        const float below = __shfl_up(p[n][0], 1 << s, LANES);
                        if (pos >= (1 << s)) p[n][0] += below;
                    }
                }
#pragma unroll
            for (int n = 0; n < N; ++n) p[n][0] = __shfl(p[n][0], lastlane, LANES);
        } else {
            float t[N][NCHUNK] = {};
            for (int hh = h0; hh < h1; ++hh) {
#pragma unroll
                for (int n = 0; n < N; ++n) {
                    float s = 0.f;
#pragma unroll
                    for (int c = 0; c < NCHUNK; ++c) s += hid[c] == hh ? p[n][c] : 0.f;  // a select: another head's NaN stays out
                    s = group_sum<LANES>(s);
#pragma unroll
                    for (int c = 0; c < NCHUNK; ++c) t[n][c] = hid[c] == hh ? s : t[n][c];
                }
            }
#pragma unroll
            for (int n = 0; n < N; ++n)
#pragma unroll
                for (int c = 0; c < NCHUNK; ++c) p[n][c] = t[n][c];
        }
    }
};

__device__ __forceinline__ bool dot_kept(int word, int head) { return (word >> (head & 31)) & 1; }

// Neighbour rows in flight per group: as many (at most 4) as keep the staged rows within 64 registers
constexpr int dot_unroll(int stage_regs) { return stage_regs * 4 <= 64 ? 4 : stage_regs * 2 <= 64 ? 2 : 1; }

// lanes one head needs at the vector width `vec`; more than a tile holds -> the entry points return BOT_E_RANGE
static bool dot_head_fits(int32_t D, int vec) { return D / vec <= kWave * kDotMaxChunk; }

// The ladder of instances over rows of H*D columns.  Kern::launch<VEC, LANES, NCHUNK>(args, blocks, stream) names and starts one
// instance of a sweep.
template <class Args, class Kern>
struct DotLaunch {
    Args a;
    hipStream_t st;
    template <int VEC, int LANES, int NCHUNK>
    void run() const {
        const int64_t blocks = (a.n_items * LANES + kBlock - 1) / kBlock;
        if (blocks == 0) return;
        Args b = a;
        const int fit = LANES * NCHUNK / (a.D / VEC);  // whole heads per tile (>= 1: dot_head_fits and the ladder below)
        b.hpt = fit < a.H ? fit : a.H;
        Kern::template launch<VEC, LANES, NCHUNK>(b, (unsigned)blocks, st);
    }
    // a row of L lanes: one tile of 2 / 4 / 6 chunks where it fits, else tiles of whole heads in the narrowest of them that holds one
    template <int VEC>
    void wide(int L) const {
        const int need = L <= kWave * kDotMaxChunk ? L : a.D / VEC;
        if (need <= 128) return run<VEC, 64, 2>();
        if (need <= 256) return run<VEC, 64, 4>();
        return run<VEC, 64, 6>();
    }
};

template <class Kern, class Args>
static void dot_dispatch(const Args& a, int vec, hipStream_t st) {
    dispatch_sweep(DotLaunch<Args, Kern>{a, st}, a.HD, vec);
}

}  // namespace bot
