"""A float64 restatement of the fused inference sweep's contract (include/bot_gnn.h bot_gat_infer_f32; csrc/infer.hip), shared by
tests/test_infer_host.py and tests/test_infer_gpu.py: the logits, the leaky ReLU, the per-(row, head) softmax, the weighted gather and
the epilogue over indptr / indices in plain torch float64; a Python restatement of the dispatch (which kernel instantiation a call
records with set_kernel) with the names counted from it; the case list that reaches every name; the graphs; the operand builders of the
exact regimes with their premises ASSERTED; the bound for seeded inputs; and the mutants of the restatement that show the checks are not
vacuous.  Nothing here calls the code under test.  Graphs, guarded placement and the constants U, EXACT_LIMIT, TINY come from
tests/attn_cases.py and tests/spmm_cases.py.

The kernels: a wavefront per work item covering all heads (`gat_infer_rows_kernel`, trips of 64 edges) or a LANES-wide group per (item,
head) (`gat_infer_heads_kernel`, trips of LANES = 8 / 16 / 32 / 64 edges); a whole row is swept once with an online softmax (running
max m, s = s __expf(m - m') + sum __expf(e - m'), the accumulators rescaled by the same factor) and normalised by 1 / s at the end; a
long row (degree above the row plan's chunk) gets (max, 1 / sum) from `gat_infer_rowstat_kernel` first, its slots gather with final
weights __expf(e - max) * (1 / sum) and `gat_infer_combine_kernel` adds the slots' partials in slot order and applies the epilogue.

Exact regimes.  "flat" logits: in every (row, head) each float32 logit either EQUALS the row's largest or lies at least 200 below it
(asserted by `assert_exact`).  __expf(0) is 1 and __expf(-200 or less) is 0 in float32, so the top set T has weight 1 each, s = |T|
exactly and, with x integers and ew multiples of 0.25, the accumulator holds S = sum over T of ew x exactly: a whole row gives
float32(S * float32(1 / |T|)), then one rounding per epilogue step (addend and shift integers, scale a power of two).  Equal logits
(T = the row) and spikes (|T| = 1: exactly ew x of the spike's source) are its two forms.  A LONG row multiplies every term by
float32(1 / |T|) BEFORE the sum, which is exact only where |T| is a power of two (the spikes, and equal logits on rows of 16, 32, 64,
128 edges): its other entries are held to the bound instead (the mask of `exact_expected`).  A rescale by __expf(-200) = 0 can leave -0.0 in an
accumulator, so zeros are compared without their sign.  "plain": el None, integers and ew multiples of 0.25: every entry exact.

Bound for seeded inputs (U = 2^-24; C0, C1: the measured error of __expf, |__expf(t) / exp(t) - 1| <= C0 + C1 |t|), per out entry,
from the lengths and magnitudes of the restatement only:

- The float32 logit: two additions and the slope's product, eta = U (2 zabs + |e|); it moves a weight by 2 eta_row at most.
- The exponentials.  Edge k's term is its own __expf(e_k - m) times every later rescale __expf(m - m'): at most `trips` calls, trips =
  ceil(deg / trip width) for a whole row and 1 for a long one, whose arguments add up to M - e_k (the running maximum only grows), each
  argument one rounded subtraction: chain_k = trips C0 + (C1 + U) (M - e_k).  The denominator is the sum of the same terms: its
  relative error is the weighted mean of the chains, den = sum_j a_j chain_j.
- The arithmetic of a weight: per trip the rescale's product, the sum's addition and the six steps of the wave reduction, the long
  rows' strided sum of ceil(deg / 256) terms, the reciprocal, the product by it and by ew: (8 trips + ceil(deg / 256) + 14) U.

      rel_k = chain_k + den + 2 eta_row + (8 trips + ceil(deg / 256) + 14) U
      E = sum_k [expm1(rel_k) |a_k ew_k x_k| + TINY |ew_k x_k|] + (deg + trips + slots + 4) U sum_k |a_k ew_k x_k|

  (one fmaf per edge, one rescale per trip, one addition per slot), then one rounding per epilogue step that is present: E <- E + U
  (|pre| + E) for the addend, E <- |scale| E + U (|pre scale| + |scale| E) for the scale, E <- E + U (|pre scale + shift| + E) for
  the shift; ReLU does not widen it.  TINY holds weights whose exponential is a subnormal number absolutely."""
import collections
import functools
import itertools
import types

import numpy as np
import torch

from tests import attn_cases as AC
from tests import spmm_cases as SC

F64 = torch.float64
U, EXACT_LIMIT, TINY = AC.U, AC.EXACT_LIMIT, AC.TINY
# __expf against float64 exp, measured on the MI355X through the kernel itself (tests/test_infer_gpu.py
# test_fast_exponential_error_measured_fp64): two-edge rows with logits (0, t), 4 000 seeded float32 t in [-87, 0], the ratio of the two
# weights against exp(t).  EXPF_C0_MEASURED: the largest relative error at |t| <= 1; EXPF_C1_MEASURED: the largest relative error / |t|
# at |t| > 1.  The constants of the bound are twice those.
EXPF_C0_MEASURED = 1.1042e-07     # 1.85 U, at t = -0.987142
EXPF_C1_MEASURED = 8.0863e-08     # 1.357 U per unit of |t|, at t = -1.49928 (at t = -85.8391 the error was 3.8048e-06, 4.43e-08 per unit)
EXPF_C0, EXPF_C1 = 2 * EXPF_C0_MEASURED, 2 * EXPF_C1_MEASURED
N_INSTANTIATIONS = 52
HEADS = AC.HEADS                                        # 1 .. 9, 12, 16, 17
SUBSETS = AC.SUBSETS
BOUNDARY_L = (8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 192, 193, 256)
DEGREES = (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257)
SPIKE = 300.0


# ------------------------------------------------------------------------------------------------ the dispatch, restated
def rows_layout(H, L, vec):
    """dispatch_infer_rows: (HL, NCHUNK, CPH), or None where the all-heads layout refuses the shape."""
    if H < 2 or H > 8 or L <= 8:
        return None
    if L > 64:
        return None if (L > 128 or vec == 4 or H > 3) else (64, 4 if H == 2 else 6, 2)
    HL = 16 if L <= 16 else (32 if L <= 32 else 64)
    nchunk = (H * HL + 63) // 64
    return None if nchunk > 4 else (HL, nchunk, 1)


def expected_kernel(H, D, vec):
    """The string set_kernel records for a call with these sizes and pick_vec's result `vec`; None: BOT_E_RANGE before any launch."""
    if D > vec * 256:
        return None
    L = -(-D // vec)
    rows = rows_layout(H, L, vec)
    if rows:
        return "bot::gat_infer_rows_kernel<%d,%d,%d,%d>" % ((vec,) + rows)
    return "bot::gat_infer_heads_kernel<%d,%d,%d>" % ((vec,) + SC._head_major(L))


def trip_width(kernel):
    """Edges per trip of the online softmax: 64 in the all-heads kernel, LANES in the head-major one."""
    return 64 if "rows" in kernel else int(kernel.split("<")[1].split(",")[1])


def all_instantiations():
    """Every name the dispatch can record, counted from the code: per VEC, the all-heads kernel with CPH = 1 takes HL = 16 with NCHUNK =
    ceil(16 H / 64) = 1, 2 (H = 2 .. 8), HL = 32 with 1 .. 4 (H = 2 .. 8), HL = 64 with 2 .. 4 (H = 2 .. 4; five chunks are refused) - 9,
    times 3 = 27; VEC 2 / 1 have the two-chunks-per-head forms <64, 4, 2> and <64, 6, 2> - 4; the head-major table has 7 entries per VEC -
    21.  27 + 4 + 21 = 52."""
    out = []
    for v in (4, 2, 1):
        out += ["bot::gat_infer_rows_kernel<%d,%d,%d,1>" % (v, hl, n) for hl, ns in ((16, (1, 2)), (32, (1, 2, 3, 4)), (64, (2, 3, 4))) for n in ns]
        if v != 4:
            out += ["bot::gat_infer_rows_kernel<%d,64,%d,2>" % (v, n) for n in (4, 6)]
        out += ["bot::gat_infer_heads_kernel<%d,%d,%d>" % ((v,) + t) for t in SC._HEAD_MAJOR]
    return tuple(sorted(out))


# ------------------------------------------------------------------------------------------------ operand layouts
Recipe = collections.namedtuple("Recipe", "off pad hx so ao", defaults=(0, 0, 0, 0, 0))
"""x and out lie `off` floats behind a 16-byte aligned address with head stride D + hx and row pitch H (D + hx) + pad (SC.Recipe);
scale and shift start `so` floats and the addend `ao` floats behind one (the addend with the same pitch and head stride)."""
RECIPES = (Recipe(), Recipe(pad=4), Recipe(hx=4), Recipe(pad=4, hx=4), Recipe(off=2), Recipe(pad=2), Recipe(hx=2), Recipe(so=2), Recipe(ao=2),
           Recipe(off=1), Recipe(pad=1), Recipe(hx=1), Recipe(so=1), Recipe(ao=1), Recipe(off=2, pad=4, hx=4), Recipe(off=1, pad=4, hx=4, so=2))


def slab(r, off=None):
    return SC.Recipe(off=r.off if off is None else off, pad=r.pad, hx=r.hx)


def case_vec(H, D, r, n_slots=0, addend=True, affine=True):
    """vec_of for the operands test_infer_gpu.py builds under recipe r: x, out (and the addend) share pitch and head stride; the
    partials start 2 n_slots H floats into the workspace, which the wrapper allocates aligned."""
    ld, hs = SC.strides(H, D, slab(r))
    offs = [4 * r.off] + ([4 * r.ao] if addend else []) + ([4 * r.so] if affine else [])
    return SC.vec_of(D, (ld, hs, (n_slots * H * 2) % 4), offs)


Case = collections.namedtuple("Case", "H D recipe kernel")


def kernel_of(case, d, epilogue=True):
    """The name a call of `case` on direction d records: pick_vec also sees the slot count (the partials' offset) and only the operands
    that are given (a call without addend, scale and shift is not bound by their offsets)."""
    return expected_kernel(case.H, case.D, case_vec(case.H, case.D, case.recipe, d.n_slots, epilogue, epilogue))


def _mk(H, D, vec, turn):
    """A case of width D whose operands give pick_vec = vec (no long rows, addend, scale and shift present): the recipes in turn."""
    ok = [r for r in RECIPES if case_vec(H, D, r) == vec]
    if not ok:
        return None
    r = ok[turn % len(ok)]
    return Case(H, D, r, expected_kernel(H, D, vec))


@functools.lru_cache(maxsize=None)
def cases():
    """Over VEC x the boundary L x HEADS: for every name the smallest and the largest H that map to it, each at the narrowest and the
    widest boundary L of the name (padded head slots and full chunks, idle lanes and full lanes); then cases until every boundary L per
    VEC and every H has occurred.  The recipes are taken in turn."""
    found = collections.defaultdict(list)
    for vec in (4, 2, 1):
        for L in BOUNDARY_L:
            for H in HEADS:
                name = expected_kernel(H, L * vec, vec)
                if name is not None:
                    found[name].append((H, L, vec))
    out, turn, seen_l, seen_h = [], itertools.count(), set(), set()
    for name in all_instantiations():
        t = found[name]
        assert t, name
        hs, ls = sorted({h for h, _, _ in t}), sorted({l for _, l, _ in t})
        picks = {(hs[0], ls[0]), (hs[-1], ls[-1]), (hs[0], ls[-1]), (hs[len(hs) // 2], ls[0])}
        for H, L in sorted(picks):
            vec = t[0][2]
            if (H, L, vec) in t and H * L * vec <= 2400:
                out.append(_mk(H, L * vec, vec, next(turn)))
                seen_l.add((vec, L)), seen_h.add(H)
    for vec in (4, 2, 1):
        for L in BOUNDARY_L:
            if (vec, L) not in seen_l:
                out.append(_mk(2 if L <= 128 else 1, L * vec, vec, next(turn)))
    for i, H in enumerate(h for h in HEADS if h not in seen_h):
        vec = (4, 2, 1)[i % 3]
        out.append(_mk(H, 17 * vec, vec, next(turn)))
    assert all(c is not None and c.kernel is not None for c in out) and {c.H for c in out} == set(HEADS)
    return tuple(dict.fromkeys(out))


def range_cases():
    """(H, D, vec) with D = vec * 256 (the widest legal) and D = vec * 256 + vec (BOT_E_RANGE, no launch)."""
    return tuple((H, v * 256 + dv, v) for v in (4, 2, 1) for H in (1, 2) for dv in (0, v))


# ------------------------------------------------------------------------------------------------ graphs
def lanes_edges(seed=23):
    """(src, dst, n_src, n_dst): a block of 21 destinations and 37 sources; in-degrees DEGREES and 2, 3, 40, the first row empty, the
    last the longest; sources drawn with replacement (parallel edges occur), edge ids in no particular order.  The positions of a row
    follow the edge ids."""
    rng = np.random.default_rng(seed)
    deg = np.array(DEGREES[:-1] + (2, 3, 40) + DEGREES[-1:])
    dst = np.repeat(np.arange(deg.size), deg)
    src = rng.integers(0, 37, dst.size)
    order = rng.permutation(dst.size)
    return torch.from_numpy(src[order]), torch.from_numpy(dst[order]), 37, int(deg.size)


def _lanes(chunk):
    import bot_amd
    src, dst, n_src, n_dst = lanes_edges()
    return bot_amd.Graph(src, dst, n_src, num_dst_nodes=n_dst, chunk=chunk)


def slots_of(d):
    """Slots per row: 1 for a whole row, the number of chunks for a long one."""
    s = torch.ones(d.n_rows, dtype=torch.int64)
    if d.n_long:
        lp = d.long_ptr.cpu().long()
        s[d.long_rows.cpu().long()] = lp[1:] - lp[:-1]
    return s


def is_long(d):
    m = torch.zeros(d.n_rows, dtype=torch.bool)
    if d.n_long:
        m[d.long_rows.cpu().long()] = True
    return m


def one_slot_plan(d, degree=7):
    """The CSC direction d with one WHOLE row of `degree` edges re-planned as a long row of exactly ONE slot (the row plan itself cuts a
    long row into two slots at least; the kernels take any plan): its item gets the next free slot and the row joins long_rows."""
    deg = AC.degrees(d)
    r = int(((deg == degree) & ~is_long(d)).nonzero()[0])
    items = d.items.clone()
    i = int(((items[:, 0] == r) & (items[:, 3] < 0)).nonzero()[0])
    items[i, 3] = d.n_slots
    dev = d.indptr.device
    out = types.SimpleNamespace(indptr=d.indptr, indices=d.indices, eid=d.eid, items=items, n_items=d.n_items, n_rows=d.n_rows, nnz=d.nnz,
                                chunk=d.chunk, n_long=d.n_long + 1, n_slots=d.n_slots + 1,
                                long_rows=torch.cat([d.long_rows, torch.tensor([r], dtype=torch.int32, device=dev)]),
                                long_ptr=torch.cat([d.long_ptr, torch.tensor([d.n_slots + 1], dtype=torch.int32, device=dev)]))
    return out


@functools.lru_cache(maxsize=None)
def graphs():
    """(name, CPU graph): the lanes graph three ways - chunk 300 (no long row, up to five trips a row), the default chunk (64: long 65,
    127, 128, 129, 257) and chunk 8 (long rows of 2, 3, 4, 5, 8, 9, 16, 17 and 33 slots) - three graphs of tests/attn_cases.py (a square
    one short and long, a block with long rows) and a graph without edges."""
    from bot_amd import _C
    whole, dflt, c8 = _lanes(300), _lanes(None), _lanes(8)
    assert whole.number_of_src_nodes() > whole.number_of_dst_nodes() and whole.number_of_edges() <= 1100
    deg = AC.degrees(whole.csc).tolist()
    assert all(k in deg for k in DEGREES) and deg[0] == 0 and deg[-1] == max(deg) == 257
    assert whole.csc.n_long == 0 and dflt.csc.chunk == _C.default_chunk(dflt.number_of_edges()) == 64
    assert sorted(AC.degrees(dflt.csc)[dflt.csc.long_rows.long()].tolist()) == [65, 127, 128, 129, 257]
    assert sorted(set(slots_of(c8.csc).tolist())) == [1, 2, 3, 4, 5, 8, 9, 16, 17, 33]
    named = dict(AC.graphs())
    return (("whole", whole), ("default", dflt), ("chunk8", c8), ("sweep128", named["sweep128"]), ("sweep8", named["sweep8"]),
            ("blocklong", named["blocklong"]), ("empty", SC._empty()))


# ------------------------------------------------------------------------------------------------ inputs
class Ops:
    """The operands of one call, compact CPU float32 tensors: x [n_src, H, D], el [n_src, H] or None, er [n_rows, H], ee [nnz, H], ew
    [nnz], addend [n_rows, H, D], scale / shift [H D] (each or None), slope, relu; d the direction, kernel the expected name."""


def _base(case, d, n_src, kernel, regime, slope, relu):
    o = Ops()
    o.case, o.d, o.n_src, o.H, o.D, o.kernel, o.regime, o.slope, o.relu = case, d, n_src, case.H, case.D, kernel, regime, slope, relu
    o.el = o.er = o.ee = o.ew = o.addend = o.scale = o.shift = None
    return o


def spike_positions(d, H, W):
    """[n_rows, H] positions (or -1 for an empty row): the spike of head h of row r is of kind (h + r) % 5 - the row's first edge, the
    last edge of trip 1, the first of trip 2, the row's last edge, the middle of the row (alone on its lane in a row of W + 1 .. 2 W - 1
    edges) - so the heads that share a chunk need different rescale factors in the same trip, and every head meets every kind."""
    ip, deg = d.indptr.cpu().long(), AC.degrees(d)
    pos = torch.full((d.n_rows, H), -1, dtype=torch.int64)
    for r in range(d.n_rows):
        n = int(deg[r])
        if n:
            kinds = (0, min(W, n) - 1, min(W, n - 1), n - 1, n // 2)
            for h in range(H):
                pos[r, h] = int(ip[r]) + kinds[(h + r) % 5]
    return pos


def flat_ops(case, d, n_src, kernel, mode, names, slope, seed, ew=False, epilogue=True, relu=False):
    """Exact regime "flat" (module docstring).  mode "equal": el, er, ee (those in `names`, integers; el zeros when absent, as the entry
    needs it) sum to the same value over each (row, head).  mode "spike": the same, and one logit per (row, head) is SPIKE above - on
    ee at `spike_positions` where ee is given, else on el at the head's own hot source (the top set is then every occurrence of that
    source in the row, or the whole row where it does not occur), else (er alone) nowhere.  x integers in -8 .. 8, ew multiples of 0.25 in
    0.25 .. 2, addend and shift integers, scale a power of two with either sign."""
    rng = np.random.default_rng(seed)
    o = _base(case, d, n_src, kernel, "flat", slope, relu)
    H, D, nnz, n = o.H, o.D, d.nnz, d.n_rows
    el, er, ee, _, _ = AC.equal_logit_inputs(d, n_src, H, names, None, None, seed, slope=slope)
    el = torch.zeros(n_src, H) if el is None else el.clone()
    if mode == "spike" and nnz:
        if ee is not None:
            pos = spike_positions(d, H, trip_width(kernel))
            live = pos >= 0
            ee[pos[live], torch.arange(H).expand(n, H)[live]] += SPIKE
        elif "el" in names:
            el[(torch.arange(H) * 7 + 3) % n_src, torch.arange(H)] += SPIKE
    o.el, o.er, o.ee = el, er, ee
    o.x = AC._ints(rng, -8, 8, (n_src, H, D))
    o.ew = torch.from_numpy(rng.integers(1, 9, nnz).astype(np.float32) / 4) if ew else None
    if epilogue:
        o.addend = AC._ints(rng, -8, 8, (n, H, D))
        o.scale = torch.from_numpy((2.0 ** rng.integers(-2, 3, H * D) * rng.choice([-1.0, 1.0], H * D)).astype(np.float32))
        o.shift = AC._ints(rng, -8, 8, (H * D,))
    assert_exact(o)
    return o


def plain_ops(case, d, n_src, kernel, seed, ew=False, epilogue=True, relu=False):
    """Exact regime "plain": el None, x, addend, shift integers, ew multiples of 0.25 in -2 .. 2 with both zeros, scale a power of two."""
    rng = np.random.default_rng(seed)
    o = _base(case, d, n_src, kernel, "plain", 0.2, relu)
    H, D = o.H, o.D
    o.x = AC._ints(rng, -8, 8, (n_src, H, D))
    if ew:
        w = rng.integers(-8, 9, d.nnz).astype(np.float32) / 4
        w[(w == 0) & (rng.random(d.nnz) < 0.5)] = -0.0
        o.ew = torch.from_numpy(w)
    if epilogue:
        o.addend = AC._ints(rng, -8, 8, (d.n_rows, H, D))
        o.scale = torch.from_numpy((2.0 ** rng.integers(-2, 3, H * D) * rng.choice([-1.0, 1.0], H * D)).astype(np.float32))
        o.shift = AC._ints(rng, -8, 8, (H * D,))
    assert_exact(o)
    return o


def normal_ops(case, d, n_src, kernel, seed, logit_scale=1.0, names=("el", "er", "ee"), ew=True, epilogue=True, relu=False, slope=0.2):
    """Seeded regime: x, addend, shift ~ N(0, 1); el, er, ee ~ N(0, 1) * logit_scale; ew ~ U(0, 1) with a quarter exact zeros; scale ~
    +-U(0.5, 2)."""
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(s, generator=gen)
    o = _base(case, d, n_src, kernel, "normal", slope, relu)
    o.tag = "normal %g" % logit_scale
    H, D, nnz, n = o.H, o.D, d.nnz, d.n_rows
    o.x = r(n_src, H, D)
    el, er, ee = r(n_src, H) * logit_scale, r(n, H) * logit_scale, r(nnz, H) * logit_scale
    o.el = el if "el" in names else torch.zeros(n_src, H)
    o.er, o.ee = er if "er" in names else None, ee if "ee" in names else None
    if ew:
        o.ew = torch.rand(nnz, generator=gen)
        o.ew[torch.rand(nnz, generator=gen) < 0.25] = 0.0
    if epilogue:
        o.addend, o.shift = r(n, H, D), r(H * D)
        o.scale = (0.5 + 1.5 * torch.rand(H * D, generator=gen)) * torch.where(torch.rand(H * D, generator=gen) < 0.5, -1.0, 1.0)
    return o


def logits32(o):
    """e in float32 in the kernel's own order, (el[src] + er[row]) + ee[k] and the slope's product: IEEE operations, bit for bit the
    kernel's logit."""
    d = o.d
    z = o.el[d.indices.cpu().long()] + (o.er[AC.rows_of(d)] if o.er is not None else 0.0)
    if o.ee is not None:
        z = z + o.ee
    return torch.where(z > 0, z, z * np.float32(o.slope))


def assert_exact(o):
    """The premises of the exact regimes, from the operands alone: integers and multiples of 0.25 of bounded size, the absolute terms
    of every sum below EXACT_LIMIT, and (flat) every logit equal to its (row, head)'s largest or at least 200 below it."""
    d = o.d
    for t in (o.x, o.addend, o.shift):
        assert t is None or bool((t == t.round()).all() and (t.abs() <= 8).all())
    assert o.ew is None or bool(((o.ew * 4) == (o.ew * 4).round()).all() and (o.ew.abs() <= 2).all())
    assert o.scale is None or bool((torch.log2(o.scale.abs()) == torch.log2(o.scale.abs()).round()).all())
    assert int(AC.degrees(d).max() if d.n_rows else 0) * 16 + 8 < EXACT_LIMIT and o.D <= 1028
    if o.regime == "flat" and d.nnz:
        e, rows = logits32(o), AC.rows_of(d)
        top = torch.full((d.n_rows, o.H), -np.inf).scatter_reduce(0, rows.view(-1, 1).expand(-1, o.H), e, "amax", include_self=True)
        gap = top[rows] - e
        assert bool(((gap == 0) | (gap >= 200)).all()) and bool(torch.isfinite(e).all())


def exact_expected(o):
    """(out float32 [n_rows, H, D], mask): the exact regimes' expected result with the roundings the contract has (module docstring),
    and the entries for which it is exact: all of them but, in the flat regime, the long rows whose top set is not a power of two."""
    d, H, D, n = o.d, o.H, o.D, o.d.n_rows
    rows, src = AC.rows_of(d), d.indices.cpu().long()
    w = torch.ones(d.nnz) if o.ew is None else o.ew
    mask = torch.ones(n, H, D, dtype=torch.bool)
    if o.regime == "flat":
        e = logits32(o)
        top = torch.full((n, H), -np.inf).scatter_reduce(0, rows.view(-1, 1).expand(-1, H), e, "amax", include_self=True)
        hot = (e == top[rows]).float()
        cnt = torch.zeros(n, H).index_add_(0, rows, hot)
        S = torch.zeros(n, H, D).index_add_(0, rows, (hot * w[:, None])[:, :, None] * o.x[src])       # exact: asserted premises
        v = S * (torch.ones(()) / cnt.clamp(min=1))[:, :, None]                                        # float32: acc * (1.f / s)
        pow2 = torch.log2(cnt.clamp(min=1)) == torch.log2(cnt.clamp(min=1)).round()
        mask = (~is_long(d)[:, None] | pow2)[:, :, None].expand(n, H, D).clone()
    else:
        v = torch.zeros(n, H, D).index_add_(0, rows, w[:, None, None] * o.x[src])
    v = _epilogue(v, o, None)
    return v + 0.0, mask


def _epilogue(v, o, mutant, slots=None):
    n, H, D = v.shape
    cast = (lambda t: t.to(v.dtype))
    sc = None if o.scale is None else cast(o.scale).view(1, H, D)
    sh = None if o.shift is None else cast(o.shift).view(1, H, D)
    if o.addend is not None:
        v = v + cast(o.addend) * (slots.view(-1, 1, 1).to(v.dtype) if mutant == 7 else 1)
    if o.relu and mutant == 9:
        v = v.clamp(min=0)
    if mutant == 8:
        v = v if sh is None else v + sh
        v = v if sc is None else v * sc
    else:
        v = v if sc is None else v * sc
        v = v if sh is None else v + sh
    if o.relu and mutant != 9:
        v = torch.where(v < 0, torch.zeros((), dtype=v.dtype), v)      # (the non-finite cases run without ReLU: fmaxf(NaN, 0) is 0)
    return v


# ------------------------------------------------------------------------------------------------ the contract, float64
MUTANTS = {1: "one neighbour dropped from one row", 2: "a head's rescale taken from its chunk neighbour", 3: "er read at the source's row",
           4: "ee indexed by edge id instead of position", 5: "ew applied before the softmax", 6: "one slot's partial of a long row omitted",
           7: "the addend added once per slot", 8: "scale and shift applied in the other order", 9: "ReLU before the affine",
           10: "absmax over short rows only"}


def mutants_of(o):
    """The mutants that apply to these operands."""
    d, out = o.d, [1]
    deg = AC.degrees(d)
    if o.el is not None:
        whole = deg[~is_long(d)]
        if o.H >= 2 and whole.numel() and int(whole.max()) > trip_width(o.kernel):
            out.append(2)
        if o.er is not None:
            out.append(3)
        if o.ee is not None:
            out.append(4)
        if o.ew is not None:
            out.append(5)
    if d.n_long:
        out.append(6)
        if o.addend is not None:
            out.append(7)
        out.append(10)
    if o.scale is not None and o.shift is not None:
        out.append(8)
    if o.relu and (o.scale is not None or o.shift is not None):
        out.append(9)
    return out


def reference(o, mutant=None):
    """The contract in float64 from the float32 operands.  A -inf logit among finite ones is a dropped edge; a NaN or +inf logit makes
    its (row, head) NaN; a non-empty (row, head) of nothing but -inf is NaN; a row without edges gives act(addend scale + shift).
    -> dict: out [n_rows, H, D], absmax (max |float32(out)|, NaN ignored), and for the bound: a, e, M, zabs [nnz, H], live, mag = sum |a ew
    x|, wx = |ew x| per edge, pre (before the scale)."""
    d, H, D, n, nnz = o.d, o.H, o.D, o.d.n_rows, o.d.nnz
    rows, src, ip, deg = AC.rows_of(d), d.indices.cpu().long(), d.indptr.cpu().long(), AC.degrees(d)
    xs = o.x.double()[src]
    w = torch.ones(nnz, dtype=F64) if o.ew is None else o.ew.double()
    res = {"mutant": mutant}
    if o.el is not None:
        er_at = (src % max(n, 1)) if mutant == 3 else rows
        ee_at = d.eid.cpu().long() if mutant == 4 else torch.arange(nnz)
        parts = [o.el[src]] + ([o.er[er_at]] if o.er is not None else []) + ([o.ee[ee_at]] if o.ee is not None else [])
        z32, z, zabs = parts[0].clone(), parts[0].double(), parts[0].double().abs()
        for p in parts[1:]:
            z32, z, zabs = z32 + p, z + p.double(), zabs + p.double().abs()
        e = torch.where(z32 > 0, z, z * float(np.float32(o.slope)))
        fin = torch.isfinite(e)
        bad = ~fin & ~torch.isneginf(e)
        idx = rows.view(-1, 1).expand(-1, H)
        M = torch.full((n, H), -np.inf, dtype=F64).scatter_reduce(0, idx, torch.where(fin, e, torch.full((), -np.inf, dtype=F64)), "amax", include_self=True)
        M = torch.where(torch.isneginf(M), torch.zeros((), dtype=F64), M)
        ex = torch.where(fin, torch.exp(torch.where(fin, e, torch.zeros((), dtype=F64)) - M[rows]), torch.zeros((), dtype=F64))
        if mutant == 5:
            ex = ex * w[:, None]
        a = ex / torch.zeros(n, H, dtype=F64).index_add_(0, rows, ex)[rows]            # 0 / 0: the all -inf (row, head) is NaN
        poisoned = torch.zeros(n, H, dtype=F64).index_add_(0, rows, bad.double()) > 0
        a = torch.where(poisoned[rows], torch.full((), np.nan, dtype=F64), a)
        res.update(e=e, M=M, zabs=zabs, fin=fin)
        if mutant == 2:
            a = _wrong_rescale(o, a, e, fin)
    else:
        a = torch.ones(nnz, H, dtype=F64)
    aw = a if mutant == 5 else a * w[:, None]
    terms = aw[:, :, None] * xs
    if mutant == 1:
        k = int((torch.nan_to_num(terms).abs().amax((1, 2)) * (deg[rows] >= 2)).argmax())
        terms = terms.clone()
        terms[k] = 0
    if mutant == 6:
        r = int(deg.argmax())
        terms = terms.clone()
        terms[ip[r] + d.chunk:min(int(ip[r]) + 2 * d.chunk, int(ip[r + 1]))] = 0
    agg = torch.zeros(n, H, D, dtype=F64).index_add_(0, rows, terms)
    res["a"], res["mag"] = a, torch.zeros(n, H, D, dtype=F64).index_add_(0, rows, torch.nan_to_num(terms).abs())
    res["wx"] = w[:, None, None].abs() * xs.abs()
    res["pre"] = agg + (o.addend.double() if o.addend is not None else 0)
    out = _epilogue(agg, o, mutant, slots_of(d))
    res["out"] = out
    keep = ~is_long(d) if mutant == 10 else torch.ones(n, dtype=torch.bool)
    m = torch.nan_to_num(out[keep].float().abs(), nan=0.0)
    res["absmax"] = float(m.max()) if m.numel() else 0.0
    return res


def _wrong_rescale(o, a, e, fin):
    """Mutant 2 on the longest whole row: one head's accumulator is rescaled with the factors of the head next to it in its chunk (h ^
    1; its sum with its own), trip by trip - the head for which that changes the weights the most."""
    d, W = o.d, trip_width(o.kernel)
    deg, ip = AC.degrees(d).clone(), d.indptr.cpu().long()
    deg[is_long(d)] = 0
    r = int(deg.argmax())
    b, n = int(ip[r]), int(deg[r])
    ev = torch.where(fin, e, torch.full((), -np.inf, dtype=F64))[b:b + n]
    best = None
    for h in range(o.H - o.H % 2):
        pair = ev[:, [h, h ^ 1]]
        m = torch.full((2,), -np.inf, dtype=F64)
        s = torch.zeros((), dtype=F64)
        coef = torch.zeros(n, dtype=F64)                   # what the head's accumulator holds of each edge
        for t in range(0, n, W):
            mn = torch.maximum(m, pair[t:t + W].amax(0))
            sc = torch.where(torch.isneginf(m), torch.zeros((), dtype=F64), torch.exp(m - mn))
            p = torch.exp(pair[t:t + W, 0] - mn[0])
            s = s * sc[0] + p.sum()
            coef[:t] *= sc[1]
            coef[t:t + W] = p
            m = mn
        moved = float((coef / s - a[b:b + n, h]).abs().sum())
        if best is None or moved > best[0]:
            best = (moved, h, coef / s)
    a = a.clone()
    a[b:b + n, best[1]] = best[2]
    return a


# ------------------------------------------------------------------------------------------------ the bound (module docstring)
def out_bound(o, ref, c0=None, c1=None):
    c0, c1 = EXPF_C0 if c0 is None else c0, EXPF_C1 if c1 is None else c1
    d, H, D, n = o.d, o.H, o.D, o.d.n_rows
    rows, src, deg = AC.rows_of(d), d.indices.cpu().long(), AC.degrees(d).double()
    lng, slots = is_long(d), slots_of(d).double()
    trips = torch.where(lng, torch.ones(n, dtype=F64), torch.ceil(deg / trip_width(o.kernel))).clamp(min=1)
    a = torch.nan_to_num(ref["a"])
    terms = (a[:, :, None] * ref["wx"])
    E = (deg + trips + slots + 4).view(-1, 1, 1) * U * ref["mag"]
    if o.el is not None:
        zero = torch.zeros((), dtype=F64)
        alive = ref["fin"] & (a > 0)
        t = torch.where(alive, ref["M"][rows] - ref["e"], zero).clamp(min=0)
        chain = torch.where(alive, trips[rows, None] * c0 + (c1 + U) * t, zero)
        den = torch.zeros(n, H, dtype=F64).index_add_(0, rows, a * chain)
        eta = torch.where(alive, U * (2 * ref["zabs"] + ref["e"].abs()), zero)
        eta_row = torch.zeros(n, H, dtype=F64).scatter_reduce(0, rows.view(-1, 1).expand(-1, H), eta, "amax", include_self=True)
        arith = (8 * trips + torch.ceil(deg / 256) + 14) * U
        rel = chain + den[rows] + 2 * eta_row[rows] + arith[rows, None]
        E = E + torch.zeros(n, H, D, dtype=F64).index_add_(0, rows, torch.expm1(rel)[:, :, None] * terms + TINY * ref["wx"])
    pre = torch.nan_to_num(ref["pre"])
    if o.addend is not None:
        E = E + U * (pre.abs() + E)
    if o.scale is not None:
        sc = o.scale.double().view(1, H, D)
        pre, E = pre * sc, sc.abs() * E + U * ((pre * sc).abs() + sc.abs() * E)
    if o.shift is not None:
        pre = pre + o.shift.double().view(1, H, D)
        E = E + U * (pre.abs() + E)
    return E + 2.0 ** -126


def check(o, got, ref, worst=None, tag=""):
    """Compare a result (out: CPU float32 [n_rows, H, D]; absmax: float or None) with the restatement: NaN exactly where the
    restatement has NaN; in the exact regimes bit for bit (zeros without their sign) on the mask of `exact_expected`; everything under the bound.
    -> the list of differences (empty: passed).  worst: dict keeping the largest error over its bound per tag."""
    bad, out, want = [], got["out"], ref["out"]
    nan = torch.isnan(want)
    if not torch.equal(torch.isnan(out), nan):
        bad.append("NaN entries: %d got, %d wanted" % (int(torch.isnan(out).sum()), int(nan.sum())))
    if o.regime in ("flat", "plain") and not bool(nan.any()):
        exp, mask = exact_expected(o)
        ne = ((out + 0.0).view(torch.int32) != exp.view(torch.int32)) & mask
        if bool(ne.any()):
            at = ne.nonzero()
            bad.append("exact: %d differ, first (index, got, want) %s" % (
                at.shape[0], [(tuple(t.tolist()), float(out[tuple(t)]), float(exp[tuple(t)])) for t in at[:4]]))
    err, bound = (out.double() - want).abs()[~nan], out_bound(o, ref)[~nan]
    if err.numel():
        if bool(torch.isnan(err).any()) or bool((err > bound).any()):
            bad.append("bound: largest error / bound %.3g" % float((err / bound).nan_to_num(nan=np.inf).max()))
        if worst is not None and not bad:
            key, ratio = getattr(o, "tag", o.regime) + tag, float((err / bound).max())
            if ratio > worst.get(key, 0.0):
                row = int((~nan).nonzero()[int((err / bound).argmax())][0])
                worst[key], worst[key + " at"] = ratio, dict(kernel=o.kernel, H=o.H, D=o.D, n_slots=o.d.n_slots, degree=int(AC.degrees(o.d)[row]),
                                                             epilogue=o.addend is not None, relu=o.relu)
    if got.get("absmax") is not None:
        own = torch.nan_to_num(out.abs(), nan=0.0)
        if got["absmax"] != (float(own.max()) if own.numel() else 0.0):
            bad.append("absmax %r is not max |out| %r" % (got["absmax"], float(own.max()) if own.numel() else 0.0))
        elif abs(got["absmax"] - ref["absmax"]) > float(out_bound(o, ref)[~nan].max() if (~nan).any() else 0):
            bad.append("absmax against the restatement")
    return bad
