// What the PNA sweeps share (spmm_pna.hip, spmm_pna_edge.hip; include/bot_gnn.h "PNA aggregation"): the aggregator and record-section
// codes, the forward's arguments (PnaArgs), the pivot row, the row epilogue behind the reduce (pna_finish: b, the aggregators, the scalers,
// the tower-major store and the backward's saved arrays) and the entry points' decode of the aggregator codes (pna_codes).  Both files
// include it BEFORE anything that switches contraction off, so that the epilogue is the same arithmetic in both.
#pragma once
#include "sweep.h"

#include <initializer_list>
#include <math.h>

namespace bot {

constexpr int kPnaMax = 8;  // aggregators, and scalers, of one call
enum PnaAgg { kMean = 0, kSum = 1, kMax = 2, kMin = 3, kStd = 4, kVar = 5 };
enum PnaSec { kG0 = 0, kC1 = 1, kMu = 2, kGmax = 3, kGmin = 4, kAmax = 5, kAmin = 6, kSecs = 7 };

template <int VEC>
__device__ __forceinline__ void ivstore_pna(int32_t* p, const int (&r)[VEC]) {
    float f[VEC];
#pragma unroll
    for (int t = 0; t < VEC; ++t) f[t] = __int_as_float(r[t]);
    vstore<VEC>(reinterpret_cast<float*>(p), f);
}

struct PnaArgs {
    const int32_t* indptr;
    const int32_t* indices;
    const int4* items;
    int64_t n_items, n_rows;
    const float* a;
    int64_t lda;
    const float* b;  // may be NULL
    int64_t ldb;
    int32_t F, Ft, A, S, pivot;
    int8_t code[kPnaMax];
    const float* scale;  // [S, n_rows], NULL: every scaler is 1
    float* out;
    int64_t ldo;
    float* saved;  // [n_rows, 2 F]: mean of a, std (0 where var == 0); may be NULL
    int64_t lds;
    int32_t* sarg;  // [n_rows, 2 F]: argmax, argmin; NULL with saved
    int64_t ldg;
    float* ws;  // six planes of [n_slots, F]: S1, S2, max, its position, min, its position
    int64_t plane;
};

// The first neighbour's row of `row`, whose positions start at `first`: the pivot (pivot == 0: row 0 of a, a constant row - what
// tools/bench_pna.py prices the pivot's gather against; any pivot gives the same sums up to rounding)
__device__ __forceinline__ const float* pna_pivot(const PnaArgs& a, int first) {
    return a.a + (int64_t)(a.pivot ? a.indices[first] : 0) * a.lda;
}

// The epilogue of VEC columns from f0 of destination `row` with n in-edges: b, the aggregators, the scalers, the tower-major store and
// the backward's saved arrays.  An empty row is all zeros (no b), its positions -1.
template <int VEC>
__device__ __forceinline__ void pna_finish(const PnaArgs& a, int row, int f0, int n, const float (&p)[VEC], const float (&s1)[VEC],
                                           const float (&s2)[VEC], const float (&mx)[VEC], const int (&am)[VEC], const float (&mn)[VEC],
                                           const int (&an)[VEC]) {
    const int t0 = f0 / a.Ft;
    float* o = a.out + (int64_t)row * a.ldo + (int64_t)t0 * a.S * a.A * a.Ft + (f0 - t0 * a.Ft);
    float vmean[VEC], vsum[VEC], vmax[VEC], vmin[VEC], vstd[VEC], vvar[VEC], mu[VEC], gate[VEC];
    int pmax[VEC], pmin[VEC];
    float bv[VEC] = {};
    if (n > 0 && a.b) vload<VEC>(bv, a.b + (int64_t)row * a.ldb + f0);
    const float fn = (float)n;
#pragma unroll
    for (int t = 0; t < VEC; ++t) {
        const float m1 = s1[t] / fn;
        const float v = s2[t] / fn - m1 * m1;
        const float var = v > 0.f ? v : (v != v ? v : 0.f);  // relu that carries a NaN
        const float sd = sqrtf(var + 1e-30f);
        const bool some = n > 0;
        mu[t] = some ? p[t] + m1 : 0.f;
        vmean[t] = some ? mu[t] + bv[t] : 0.f;
        vsum[t] = some ? s1[t] + fn * p[t] + fn * bv[t] : 0.f;
        vmax[t] = some ? mx[t] + bv[t] : 0.f;
        vmin[t] = some ? mn[t] + bv[t] : 0.f;
        vstd[t] = some ? sd : 0.f;
        vvar[t] = some ? var : 0.f;
        gate[t] = some && var > 0.f ? sd : 0.f;
        pmax[t] = some ? am[t] : -1;
        pmin[t] = some ? an[t] : -1;
    }
    for (int s = 0; s < a.S; ++s) {
        const float sc = (n > 0 && a.scale) ? a.scale[(int64_t)s * a.n_rows + row] : 1.f;
        for (int g = 0; g < a.A; ++g) {
            const int code = a.code[g];
            float r[VEC];
#pragma unroll
            for (int t = 0; t < VEC; ++t) {
                float v = vmean[t];
                v = code == kSum ? vsum[t] : v;
                v = code == kMax ? vmax[t] : v;
                v = code == kMin ? vmin[t] : v;
                v = code == kStd ? vstd[t] : v;
                v = code == kVar ? vvar[t] : v;
                r[t] = n > 0 ? sc * v : 0.f;
            }
            vstore<VEC>(o + (int64_t)(s * a.A + g) * a.Ft, r);
        }
    }
    if (a.saved) {
        vstore<VEC>(a.saved + (int64_t)row * a.lds + f0, mu);
        vstore<VEC>(a.saved + (int64_t)row * a.lds + a.F + f0, gate);
        ivstore_pna<VEC>(a.sarg + (int64_t)row * a.ldg + f0, pmax);
        ivstore_pna<VEC>(a.sarg + (int64_t)row * a.ldg + a.F + f0, pmin);
    }
}

// The aggregator codes of a call (a HOST array) into code[], and the record's sections they need into off[] (-1: absent) in the fixed
// order g0, c1, mean, gmax, gmin, argmax, argmin, each F words.  Returns the number of sections, or a negative error code.
static int pna_codes(const char* who, const int32_t* aggs, int32_t A, int32_t F, int8_t (&code)[kPnaMax], int32_t (&off)[kSecs]) {
    BOT_REQUIRE(A >= 1 && A <= kPnaMax, BOT_E_RANGE, "%s: A=%d aggregators (1 .. %d)", who, A, kPnaMax);
    BOT_REQUIRE(aggs, BOT_E_NULL, "%s: aggs is NULL", who);
    bool need[kSecs] = {};
    for (int g = 0; g < kPnaMax; ++g) code[g] = 0;
    for (int g = 0; g < A; ++g) {
        BOT_REQUIRE(aggs[g] >= kMean && aggs[g] <= kVar, BOT_E_RANGE, "%s: unknown aggregator code %d (0 mean, 1 sum, 2 max, 3 min, 4 std, 5 var)",
                    who, aggs[g]);
        code[g] = (int8_t)aggs[g];
        if (aggs[g] == kMean || aggs[g] == kSum) need[kG0] = true;
        if (aggs[g] == kStd || aggs[g] == kVar) need[kC1] = need[kMu] = true;
        if (aggs[g] == kMax) need[kGmax] = need[kAmax] = true;
        if (aggs[g] == kMin) need[kGmin] = need[kAmin] = true;
    }
    int n = 0;
    for (int q = 0; q < kSecs; ++q) off[q] = need[q] ? F * n++ : -1;
    return n;
}

}  // namespace bot
