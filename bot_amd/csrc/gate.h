// The per-channel sigmoid gate that spmm_gate.hip and spmm_gate_edge.hip share (include/bot_gnn.h "Gated aggregation"): one exponential
// and two true divisions, the complement formed directly, so g, gbar and g' = g gbar keep a RELATIVE error bound in both tails and
// s = 0, s >= 105 and s <= -105 are exact bit for bit.  Includes smx.h, which switches contraction off for the rest of the including
// file: include it last.
#pragma once
#include "smx.h"

namespace bot {

struct Gate {
    float g, gbar;
};

__device__ __forceinline__ Gate gate_of(float s) {
    const float e = smx_exp(-fabsf(s));
    const float d = 1.f + e;
    const bool pos = s >= 0.f;
    return Gate{(pos ? 1.f : e) / d, (pos ? e : 1.f) / d};
}

}  // namespace bot
