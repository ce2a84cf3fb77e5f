"""Float64 restatements of the SpMM sweeps' contracts (include/bot_gnn.h bot_spmm_f32, bot_spmm_dot_f32, bot_spmm_dot_halves_f16,
bot_spmm_bcast_f32, bot_spmm_bcast_halves_f16, bot_spmm_dot_bcast_f32 and the absmax by-product; the docstrings of bot_amd/_C.py), shared
by tests/test_spmm_host.py and tests/test_spmm_gpu.py: plain gathers and sums over indptr / indices, the halves encoding in numpy
float32 / float16, a Python restatement of the dispatch of csrc/spmm.hip (which kernel instantiation a call records with set_kernel),
the list of cases that reaches every instantiation, the graphs, the operand placement (views into guarded allocations), the two input
regimes with their premises ASSERTED, the bounds for seeded inputs and the mutants of the restatement that show the checks are not
vacuous.  Nothing here calls the code under test.

The kernels (csrc/spmm.hip): a lane group (or a wavefront covering all heads, the "rows" layout; or flat 16-byte lanes) per work item,
lanes across the feature dimension, VEC = 4 / 2 / 1 floats per lane chosen by pick_vec from the width, strides and base addresses; the
neighbours of a row are summed in position order with one fmaf each, so a row of `deg` edges costs deg roundings per element; a long
row (degree above the row plan's chunk) is cut into slots whose partial sums spmm_combine_kernel adds in slot order.

Bounds for seeded inputs (U = 2^-24), entry for entry, from lengths and magnitudes of the restatement only:

`out`: the kernel evaluates acc = fmaf(w_k, x_k, acc) for the deg (times h heads for spmm_dot_bcast, where one accumulator takes all
heads of an edge) terms of a row, one rounding each, then at most one addition of the addend; a long row adds its n_slots partials
instead, n_slots - 1 further roundings while each partial has at most chunk terms, which is no more roundings on any path from a term
to the result than deg + 1.  The standard bound of a recursive sum of n terms with n roundings, (1 + U)^n - 1 <= n U / (1 - n U),
applied to the absolute terms gives |out - ref| <= (deg h + 2) U (sum |w x| + |addend|): the + 2 covers the addend's addition and the
(1 - n U) denominator (n U < 2^-13 here).

`dot`: D fmaf roundings in one lane's chain and the butterfly's additions, at most D + 1 on any path for the widths here (a lane holds
VEC * NCHUNK elements, the reduction over LANES lanes adds log2(LANES) roundings, and VEC * NCHUNK + log2(LANES) <= D + 1 for every
dispatched layout): |dot - ref| <= (D + 1) U sum |x y|.

decoded halves (store_halves): z = v s with s a power of two is exact; h1 = rn16(z) leaves r = z - h1 with |r| <= 2^-11 |z|, exact in
float32; 2048 r is exact and h2 = rn16(2048 r) is off by at most 2^-11 |2048 r| <= 2^-11 |z|, or by half the subnormal spacing, 2^-25,
where 2048 r is below 2^-14; decoded (h1 + h2 / 2048) / s is therefore within 2^-22 |v| + 2^-36 / s of v, and v itself within the `out`
bound of the restatement: |dec - ref| <= B + 2^-22 (|ref| + B) + 2^-36 / s."""
import collections
import functools
import itertools

import numpy as np
import torch

from tests import _oracle_backend as OB
from tests import attn_cases as AC

F64 = torch.float64
U = AC.U
EXACT_LIMIT = AC.EXACT_LIMIT     # multiples of 0.25 whose absolute terms add up to less than 2^22 are exact in float32 in any order
GUARD = 64                       # floats (or halves) of guard in front of and behind every operand view
SENTINEL32 = 0x7FC5A5A5                  # a quiet NaN with a payload no sum produces (as int32)
SENTINEL16 = 0x7E5A                      # the same for fp16 outputs (as int16)
ENTRIES = ("spmm", "spmm_dot", "spmm_dot_halves", "spmm_bcast", "spmm_bcast_halves", "spmm_dot_bcast")
ONE_TILE = ENTRIES[1:]           # D (hpiece) <= vec * 256, BOT_E_RANGE beyond
WPERMS = (None, "eid", "random")
BOUNDARY_L = (8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 192, 193, 256, 257)
LANES_DEGREES = (0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129)
LANES_CHUNK = 32


# ------------------------------------------------------------------------------------------------ the dispatch, restated
def vec_of(D, strides, byte_offsets):
    """common.h pick_vec: the widest of 4 / 2 / 1 that divides D and every stride and to whose 4 * v bytes every base is aligned."""
    for v in (4, 2):
        if D % v == 0 and all(s % v == 0 for s in strides) and all(b % (4 * v) == 0 for b in byte_offsets):
            return v
    return 1


def _head_major(L):
    for lim, ln, nc in ((8, 8, 1), (16, 16, 1), (32, 32, 1), (64, 64, 1), (128, 64, 2), (192, 64, 3)):
        if L <= lim:
            return ln, nc
    return 64, 4


def _rows_layout(H, L, vec):
    """dispatch_spmm_rows / dispatch_spmm_dot_rows: (HL, NCHUNK, CPH) or None where the all-heads layout refuses the shape."""
    if H < 2 or L <= 8:
        return None
    if L > 64:
        return None if (L > 128 or vec == 4 or H > 3) else (64, 4 if H == 2 else 6, 2)
    HL = 16 if L <= 16 else (32 if L <= 32 else 64)
    nchunk = (H * HL + 63) // 64
    return None if nchunk > 4 else (HL, nchunk, 1)


def expected_kernel(entry, H, D, vec, weighted=True, flat=False, hpiece=None):
    """The string set_kernel records for a call of `entry` (csrc/spmm.hip), or None where the entry returns BOT_E_RANGE before any
    launch.  `vec`: what pick_vec gives for the call's operands (vec_of).  `flat`: the flat layout is asked for (bot_spmm_set_layout(1))
    AND the operands allow it (head strides == D, x 16-byte aligned, ldx a multiple of 4 covering the tail float4)."""
    L = -(-D // vec)
    if entry == "spmm":
        if flat and weighted and 2 <= H <= 4 and D % 4 != 0 and D >= 4 and H * D <= 1024:
            return "bot::spmm_flat_kernel<%d,%d>" % ((H * D + 255) // 256, 3 if H <= 3 else 4)
        rows = _rows_layout(H, L, vec) if weighted else None
        if rows:
            return "bot::spmm_rows_kernel<%d,%d,%d,%d>" % ((vec,) + rows)
        return "bot::spmm_kernel<%d,%d,%d,%s>" % ((vec,) + _head_major(L) + ("true" if weighted else "false",))
    if entry in ("spmm_dot", "spmm_dot_halves"):
        if D > vec * 256 or (entry == "spmm_dot_halves" and H < 2):
            return None
        rows = _rows_layout(H, L, vec)
        if rows:
            return "bot::spmm_dot_rows_kernel<%d,%d,%d,%d>" % ((vec,) + rows)
        return None if entry == "spmm_dot_halves" else "bot::spmm_dot_kernel<%d,%d,%d>" % ((vec,) + _head_major(L))
    if entry in ("spmm_bcast", "spmm_bcast_halves", "spmm_dot_bcast"):
        width = D if entry != "spmm_bcast_halves" else hpiece
        if not 1 <= H <= 4 or D > 1024 or width > vec * 256 or width < D:
            return None
        L = -(-width // vec)
        ln, nc = (16, 1) if L <= 16 else ((32, 1) if L <= 32 else ((64, 1) if L <= 64 else ((64, 2) if L <= 128 else (64, 4))))
        return "bot::spmm_%sbcast_kernel<%d,%d,%d,%d>" % ("dot_" if entry == "spmm_dot_bcast" else "", vec, ln, nc, H)
    raise ValueError(entry)


_HEAD_MAJOR = ((8, 1), (16, 1), (32, 1), (64, 1), (64, 2), (64, 3), (64, 4))
_BCAST = ((16, 1), (32, 1), (64, 1), (64, 2), (64, 4))


def _rows_names(kind):
    """The all-heads instantiations, counted from the dispatchers: per VEC, HL = 16 takes NCHUNK = ceil(16 H / 64) = 1 .. 4 (H = 2 .. 16),
    HL = 32 takes 1 .. 4 (H = 2 .. 8), HL = 64 takes 2 .. 4 (H = 2 .. 4; NCHUNK = 1 would be H = 1) - 11 - and VEC = 2 / 1 have the two
    two-chunk-per-head forms <64, 4, 2> and <64, 6, 2>: 3 * 11 + 2 * 2 = 37."""
    out = []
    for v in (4, 2, 1):
        out += [(v, 16, n, 1) for n in (1, 2, 3, 4)] + [(v, 32, n, 1) for n in (1, 2, 3, 4)] + [(v, 64, n, 1) for n in (2, 3, 4)]
        if v != 4:
            out += [(v, 64, 4, 2), (v, 64, 6, 2)]
    return ["bot::spmm_%srows_kernel<%d,%d,%d,%d>" % ((kind,) + t) for t in out]


@functools.lru_cache(maxsize=None)
def entry_instantiations(entry):
    """Every name `entry` can record over its legal domain, counted from the dispatch code (not from running it)."""
    if entry == "spmm":
        hm = ["bot::spmm_kernel<%d,%d,%d,%s>" % (v, ln, nc, w) for v in (4, 2, 1) for ln, nc in _HEAD_MAJOR for w in ("true", "false")]
        flat = ["bot::spmm_flat_kernel<%d,%d>" % (nc, hm_) for nc in (1, 2, 3, 4) for hm_ in (3, 4)]
        return tuple(hm + _rows_names("") + flat)                                   # 42 + 37 + 8
    if entry == "spmm_dot":
        return tuple(["bot::spmm_dot_kernel<%d,%d,%d>" % (v, ln, nc) for v in (4, 2, 1) for ln, nc in _HEAD_MAJOR] + _rows_names("dot_"))   # 21 + 37
    if entry == "spmm_dot_halves":
        return tuple(_rows_names("dot_"))                                           # the 37 again, with the halves store
    kind = "dot_" if entry == "spmm_dot_bcast" else ""
    return tuple("bot::spmm_%sbcast_kernel<%d,%d,%d,%d>" % (kind, v, ln, nc, hb) for v in (4, 2, 1) for ln, nc in _BCAST for hb in (1, 2, 3, 4))   # 60


def all_instantiations():
    """Every kernel name the seven entry points can record: 42 + 8 + 37 + 21 + 37 + 60 + 60 = 265."""
    return tuple(sorted({n for e in ENTRIES for n in entry_instantiations(e)}))


# ------------------------------------------------------------------------------------------------ operand layouts
Recipe = collections.namedtuple("Recipe", "off pad hx round4", defaults=(0, 0, 0, False))
"""Where an [n, H, D] operand lies in its allocation: `off` floats behind a 16-byte aligned address (0 / 1 / 2 = 0, 4, 8 bytes), head
stride D + hx, row pitch H (D + hx) + pad; round4: the flat kernel's layout, head stride D and the pitch H D rounded up to 4, + pad."""
RECIPES = (Recipe(), Recipe(pad=4), Recipe(hx=4), Recipe(off=2), Recipe(pad=2), Recipe(hx=2), Recipe(off=1), Recipe(pad=1), Recipe(hx=1),
           Recipe(off=2, pad=4, hx=4), Recipe(off=1, pad=4, hx=4))
FLAT_RECIPES = (Recipe(round4=True), Recipe(pad=4, round4=True))


def strides(H, D, r):
    """(row pitch, head stride) of an [n, H, D] operand under recipe r, as _C._slab reports them (H == 1: head stride D)."""
    if r.round4:
        return (H * D + 3) // 4 * 4 + r.pad, D
    return H * (D + r.hx) + r.pad, (D + r.hx if H > 1 else D)


def case_vec(entry, H, D, r, addend=False):
    """vec_of for the operands test_spmm_gpu.py builds under recipe r (every float operand of a call shares r; workspaces and the
    outputs the wrappers allocate themselves are aligned and contiguous)."""
    ld, hs = strides(H, D, r)
    if entry in ("spmm", "spmm_dot", "spmm_dot_halves"):
        return vec_of(D, (ld, hs), (4 * r.off,))
    if entry in ("spmm_bcast", "spmm_bcast_halves"):     # x [n, D] with pitch D + pad; out: [H, n, D] or [n, H, D], contiguous
        return vec_of(D, (D + r.pad,), (4 * r.off,))
    return vec_of(D, (D + r.pad,), (4 * r.off,))         # spmm_dot_bcast: x contiguous [H, n, D] at off; y and out with pitch D + pad


Case = collections.namedtuple("Case", "entry H D recipe weighted flat hpiece head_outer kernel boundary")


def _halves_piece(D, crossing=False):
    return (D + 3) // 4 * 4 + (8 if crossing else 0)


def _mk(entry, H, D, r, weighted=True, flat=False, hpiece=None, boundary=False, i=0):
    if entry == "spmm_bcast_halves" and hpiece is None:
        hpiece = _halves_piece(D)
    vec = case_vec(entry, H, D, r)
    name = expected_kernel(entry, H, D, vec, weighted, flat, hpiece)
    return None if name is None else Case(entry, H, D, r, weighted, flat, hpiece, i % 2 == 0, name, boundary)


_WIDTHS = tuple(sorted({v * L for v in (1, 2, 4) for L in (3, 8, 9, 12, 16, 17, 24, 32, 33, 48, 64, 65, 100, 128, 129, 160, 192, 193, 250, 256)}
                       | {5, 7, 15, 30, 50, 62, 63, 125, 250, 257, 333}))


@functools.lru_cache(maxsize=None)
def cases():
    """The case list: for every (entry, name of entry_instantiations(entry)) the narrowest (D, H) that reaches it, the recipes taken in
    turn so that every pitch, head stride and base offset occurs; then the boundary widths L of each table per VEC; the n_tiles = 1, 2, 3
    forms of spmm_kernel; D = vec * 256 of the one-tile entries; and bot_spmm_bcast_halves with hpiece past a lane-table boundary that D
    stays below.  All reached in-process: head-major kernels with H == 1, w None, L <= 8 or shapes the rows layout refuses; the flat
    kernel through _C.SPMM_LAYOUT = "flat"."""
    out, turn = [], itertools.count()
    for entry in ENTRIES:
        found = collections.defaultdict(list)
        heads = range(1, 17) if entry in ("spmm", "spmm_dot", "spmm_dot_halves") else range(1, 5)
        for D in _WIDTHS:
            for H in heads:
                for weighted, flat in ((True, False), (False, False), (True, True)) if entry == "spmm" else ((True, False),):
                    for ri, r in enumerate(FLAT_RECIPES if flat else RECIPES):
                        c = _mk(entry, H, D, r, weighted, flat, i=ri)
                        if c is not None and (flat == ("flat" in c.kernel)) and (H * D <= 1100 or "bcast" in entry):
                            found[c.kernel].append(c)
        for name in entry_instantiations(entry):
            cands = found[name]
            assert cands, (entry, name)
            D0, H0 = cands[0].D, cands[0].H                # narrowest first (the loops above ascend in D, then H)
            same = [c for c in cands if (c.D, c.H) == (D0, H0)]
            out.append(same[next(turn) % len(same)])
    for entry in ENTRIES:                                   # the boundary widths of each table
        for vec in (4, 2, 1):
            for L in BOUNDARY_L:
                D = L * vec
                r = Recipe() if vec_of(D, (), ()) == vec else Recipe(off={2: 2, 1: 1}[vec])
                for H in {"spmm": (1, 2), "spmm_dot": (1, 2), "spmm_dot_halves": (2,)}.get(entry, (2,)):
                    if D > 1028:
                        continue
                    c = _mk(entry, H, D, r, boundary=True, i=L)
                    if c is not None:
                        assert case_vec(entry, H, D, r) == vec
                        out.append(c)
    out += [_mk("spmm", 1, 250, Recipe(off=1), boundary=True), _mk("spmm", 1, 520, Recipe(off=1), boundary=True),      # n_tiles 1, 3 (vec 1)
            _mk("spmm", 1, 1026, Recipe(), boundary=True), _mk("spmm", 2, 1028, Recipe(), False, boundary=True)]     # n_tiles 3 (vec 2), 2 (vec 4)
    for D, hp in ((60, 68), (30, 36), (15, 20), (124, 132), (62, 68), (31, 36), (252, 260)):   # hpiece crosses 16 / 32 / 64 lanes, D does not
        for H in (1, 3):
            out.append(_mk("spmm_bcast_halves", H, D, Recipe(), hpiece=hp, boundary=True))
    assert all(c is not None for c in out)
    return tuple(out)


def range_cases():
    """(entry, H, D, vec) just past one launch tile, D = vec * 256 + vec: BOT_E_RANGE, no launch."""
    return tuple((e, 2, v * 256 + v, v) for e in ONE_TILE for v in (4, 2, 1) if v * 256 + v <= 1024 or e in ("spmm_dot", "spmm_dot_halves"))


def groups():
    """(entry, vec) -> cases: the parametrisation of tests/test_spmm_gpu.py."""
    out = collections.defaultdict(list)
    for c in cases():
        out[(c.entry, int(c.kernel.split("<")[1].split(",")[0]) if "flat" not in c.kernel else 0)].append(c)
    return dict(out)


# ------------------------------------------------------------------------------------------------ graphs
def lanes_edges(seed=11):
    """(src, dst, n_src, n_dst) of the "spmm lanes" graph: 24 destinations and 26 sources; in-degrees AND out-degrees include 0, 1, 3, 4,
    5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129 (the batch of four and its tail, every LANES fetch width one short,
    exact and one past); node 0 has no edge on either side and the last node of either side has the most (300); stubs are paired at
    random, so parallel edges occur; edge ids in no particular order."""
    rng = np.random.default_rng(seed)
    din = np.array(LANES_DEGREES + (2, 6, 11, 300))
    dout = np.array(LANES_DEGREES + (6, 6, 6, 1, 0, 300))
    assert din.sum() == dout.sum() and din[0] == dout[0] == 0 and din.argmax() == din.size - 1 and dout.argmax() == dout.size - 1
    dst = np.repeat(np.arange(din.size), din)
    src = rng.permutation(np.repeat(np.arange(dout.size), dout))
    order = rng.permutation(dst.size)
    return torch.from_numpy(src[order]), torch.from_numpy(dst[order]), int(dout.size), int(din.size)


def _lanes(chunk):
    import bot_amd
    src, dst, n_src, n_dst = lanes_edges()
    return bot_amd.Graph(src, dst, n_src, num_dst_nodes=n_dst, chunk=chunk)


def _empty():
    import bot_amd
    e = torch.zeros(0, dtype=torch.int64)
    return bot_amd.Graph(e, e, 9, num_dst_nodes=5, chunk=None)


@functools.lru_cache(maxsize=None)
def graphs():
    """(name, CPU graph) with the row classes asserted: the lanes graph with chunk 32 (long rows: 33, 63, 64 = 2 chunks exactly, 65, 127,
    128 = 4 chunks exactly, 129 and the last row, 300), with chunk 300 (no long row; the default chunk of a graph this small is 64, which
    cannot leave rows of 65 .. 300 edges whole) and with that default chunk (long: 65, 127, 128, 129, 300), the graphs of tests/attn_cases.py
    whose row classes fit (the sweep graph short and long, a square with long rows in front, a block), and a graph without edges."""
    from bot_amd import _C, blocked
    small, whole, dflt = _lanes(LANES_CHUNK), _lanes(300), _lanes(None)
    assert dflt.csc.chunk == _C.default_chunk(dflt.number_of_edges()) == 64
    assert sorted(AC.degrees(dflt.csr)[dflt.csr.long_rows.long()].tolist()) == [65, 127, 128, 129, 300]
    n_edges = small.number_of_edges()
    assert n_edges <= 3000 and small.number_of_src_nodes() != small.number_of_dst_nodes()
    pairs = torch.stack([small._src, small._dst], 1)
    assert torch.unique(pairs, dim=0).shape[0] < n_edges                                   # duplicate edges
    for g in (small, whole):
        for d in (g.csc, g.csr):
            deg = AC.degrees(d).tolist()
            assert all(k in deg for k in LANES_DEGREES) and deg[0] == 0 and deg[-1] == max(deg) == 300 and deg.count(300) == 1
    for d in (small.csc, small.csr):
        longs = sorted(AC.degrees(d)[d.long_rows.long()].tolist())
        assert longs == [33, 63, 64, 65, 127, 128, 129, 300] and d.n_rows - 1 in d.long_rows.tolist()
    assert whole.csc.n_long == 0 and whole.csr.n_long == 0
    named = dict(AC.graphs())
    out = [("lanes32", small), ("lanes300", whole), ("lanes", dflt)] + [(k, named[k]) for k in ("sweep8", "sweep128", "square17long", "blocklong")]
    out.append(("empty", _empty()))
    for name, g in out:
        for d in (g.csc, g.csr):
            assert d.nnz < blocked.MIN_MEAN_DEGREE * max(d.n_rows, 1), name                # far from the blocked sweep
    return tuple(out)


def graphs_for(case, i):
    """The names of the graphs the i-th case runs on: the boundary widths on the lanes graph with long rows; the widest (D >= 513) on
    the lanes graph with and without long rows; every other case on all three lanes graphs and two of the four small graphs in turn."""
    if case.boundary:
        return ("lanes32",)
    if case.D >= 513:
        return ("lanes32", "lanes300")
    small = ("sweep8", "sweep128", "square17long", "blocklong")
    return ("lanes32", "lanes300", "lanes", small[i % 4], small[(i + 1 + i // 4) % 4] if (i + 1 + i // 4) % 4 != i % 4 else small[(i + 2) % 4])


def variant(i, gi):
    """(wperm kind, with addend, seed) of the i-th case on its gi-th graph: the three wperm kinds and both addend states in turn, so that
    every case meets all of them over its graphs, and every one of them on the lanes graph over a group's cases."""
    return WPERMS[(i + gi) % 3], (i + gi // 3 + gi) % 2 == 0, 1000 * gi + i


def direction(g, entry):
    """(direction, number of nodes its indices name, the graph's own position map or None): the forward entries sweep the CSC, the fused
    backwards the CSR with the CSC positions reached through csr2csc, as the layers do."""
    if entry in ("spmm", "spmm_bcast", "spmm_bcast_halves"):
        return g.csc, g.number_of_src_nodes(), g.csc.eid
    return g.csr, g.number_of_dst_nodes(), g.csr2csc


# ------------------------------------------------------------------------------------------------ inputs
class Ops:
    """The operands of one call, compact CPU float32 tensors: x [n, H, D] ([n, D] for the bcast forward, [H, n, D] for its backward), w
    [nnz, H] or None, wperm int32 [nnz] or None, y [n_rows, H, D] ([n_rows, D]), addend [n_rows, H, D] or None, hscale [2], hpiece."""


def _rng(seed):
    return np.random.default_rng(seed)


def make_ops(case, d, n_cols, own_perm, regime, seed, wperm=None, addend=False):
    """Operands of `case` on direction d.  regime "exact": x, y, addend integers in -8 .. 8, w multiples of 0.25 in -2 .. 2 with both
    zeros, and one head whose weight is 0 on every edge of the first row of two or more edges.  regime "normal": x, y, addend ~ N(0, 1), w
    ~ U(0, 1) with a quarter set to exact 0.  The heads' weights are drawn independently, so no two heads share a weight on more than a
    few edges (mutant 3).  o.skip (False here): the call runs with the zero-skip on, see reference.  wperm: None, "eid" (the direction's own position map) or "random"."""
    rng, o = _rng(seed), Ops()
    H, D, nnz, n_rows = case.H, case.D, d.nnz, d.n_rows
    o.case, o.d, o.regime, o.hpiece = case, d, regime, case.hpiece
    xs = {"spmm_bcast": (n_cols, D), "spmm_bcast_halves": (n_cols, D), "spmm_dot_bcast": (H, n_cols, D)}.get(case.entry, (n_cols, H, D))
    ys = (n_rows, D) if case.entry == "spmm_dot_bcast" else (n_rows, H, D)
    if regime == "exact":
        draw = lambda s: torch.from_numpy(rng.integers(-8, 9, s).astype(np.float32))
        w = rng.integers(-8, 9, (nnz, H)).astype(np.float32) / 4
        w[(w == 0) & (rng.random((nnz, H)) < 0.5)] = -0.0
    else:
        draw = lambda s: torch.from_numpy(rng.standard_normal(s).astype(np.float32))
        w = rng.random((nnz, H)).astype(np.float32)
        w[rng.random((nnz, H)) < 0.25] = 0.0
    o.x, o.y = draw(xs), (draw(ys) if "dot" in case.entry else None)
    o.addend = draw((n_rows, H, D)) if addend else None
    assert not addend or case.entry == "spmm"
    o.wperm = {None: None, "eid": own_perm.cpu().to(torch.int32), "random": AC.random_perm(nnz, seed + 1)}[wperm]
    perm = AC._perm(o.wperm, nnz)
    deg, ip = AC.degrees(d), d.indptr.cpu().long()
    if bool((deg >= 2).any()):
        r = int((deg >= 2).nonzero()[0])
        w[perm[ip[r]:ip[r + 1]].numpy(), H - 1] = 0.0                                      # a head that is dropped on a whole row
        if regime == "exact":
            w[perm[ip[r]].item(), H - 1] = -0.0
    o.w = torch.from_numpy(w) if case.weighted else None
    out = reference(o)["out"]
    o.hscale = OB._pow2_scale(float(out.abs().max()) if out.numel() else 0.0) if "halves" in case.entry else None
    if regime == "exact":
        assert_exact(o)
    return o


def assert_exact(o):
    """The premises of the exact regime, from the restatement: every operand is a multiple of 0.25 (x, y, addend: integers), and the
    absolute terms of every sum stay below 2^22 (2^24 for the integer dot products), so any order of float32 additions is exact; the halves'
    scale is a power of two that puts the largest |out| in [2^13, 2^14], so z = v s is exact and h1, h2 are exact functions of v."""
    for t in (o.x, o.y, o.addend):
        assert t is None or bool((t == t.round()).all() and (t.abs() <= 8).all())
    assert o.w is None or bool(((o.w * 4) == (o.w * 4).round()).all() and (o.w.abs() <= 2).all())
    ref = reference(o, absolute=True)
    assert float(ref["out"].max() if ref["out"].numel() else 0) < EXACT_LIMIT
    assert ref["dot"] is None or float(ref["dot"].max() if ref["dot"].numel() else 0) < 2.0 ** 24
    assert AC.degrees(o.d).max() <= 300 and o.case.D <= 1028
    if o.hscale is not None:
        s = float(o.hscale[0])
        assert np.log2(s) == round(np.log2(s)) and float(reference(o)["out"].abs().max()) * s <= 2.0 ** 14


# ------------------------------------------------------------------------------------------------ the contracts, float64
MUTANTS = {1: "one neighbour dropped from one row", 2: "the last element of a head's slab zeroed", 3: "the weights of two heads swapped on one edge",
           4: "wperm ignored", 5: "one slot's partial of a long row omitted", 6: "the addend added twice on long rows",
           7: "dot written at k instead of wperm[k]", 8: "halves padding left unwritten", 9: "absmax taken over short rows only"}


def mutants_of(o):
    """The mutants that apply to these operands (a swap needs two heads, wperm mutants a non-identity wperm, slot mutants long rows...)."""
    e, out = o.case.entry, [1, 2]
    if o.case.H >= 2 and o.w is not None:
        out.append(3)
    if o.wperm is not None and o.w is not None:
        out.append(4)
    if o.d.n_long:
        out.append(5)
        if o.addend is not None:
            out.append(6)
        if e == "spmm_dot":
            out.append(9)
    if o.wperm is not None and "dot" in e:
        out.append(7)
    if e == "spmm_bcast_halves" and o.hpiece > o.case.D:
        out.append(8)
    return out


def reference(o, mutant=None, absolute=False):
    """The contract of o.case.entry in float64 from the float32 operands: {"out": [n_rows, H, D] ([n_rows, 1, D] for spmm_dot_bcast),
    "dot": [nnz, H] in RECORD order (NaN where nothing is written) or None, "absmax": max |float32(out)|, "terms": the sum of the absolute
    terms per out entry (the bounds' magnitude), "dterms": the same per dot entry}.  absolute: out and dot of the absolute values (the
    exact regime's premise).  mutant: one of MUTANTS, each placed where it changes the result the most."""
    c, d = o.case, o.d
    H, D, nnz, n_rows = c.H, c.D, d.nnz, d.n_rows
    rows, src = AC.rows_of(d), d.indices.cpu().long()
    perm = AC._perm(None if mutant == 4 else o.wperm, nnz)
    x = o.x.double()
    if c.entry in ("spmm_bcast", "spmm_bcast_halves"):
        xs = x[src][:, None, :].expand(nnz, H, D)
    elif c.entry == "spmm_dot_bcast":
        xs = x[:, src].permute(1, 0, 2)
    else:
        xs = x[src]
    wk = o.w.double()[perm] if o.w is not None else torch.ones(nnz, H, dtype=F64)
    deg, ip = AC.degrees(d), d.indptr.cpu().long()
    if mutant == 3:
        k = int(((wk[:, 0] - wk[:, 1]).abs() * xs[:, :2].abs().amax((1, 2))).argmax())
        wk = wk.clone()
        wk[k, 0], wk[k, 1] = wk[k, 1].clone(), wk[k, 0].clone()
    terms = wk[:, :, None] * xs
    if mutant == 1:
        k = int((terms.abs().amax((1, 2)) * (deg[rows] >= 2)).argmax())
        terms = terms.clone()
        terms[k] = 0
    if mutant == 5:                                                                        # the second slot of the longest row
        r = int(deg.argmax())
        terms = terms.clone()
        terms[ip[r] + d.chunk:min(int(ip[r]) + 2 * d.chunk, int(ip[r + 1]))] = 0
    aterms = terms.abs()
    if c.entry == "spmm_dot_bcast":
        terms, aterms = terms.sum(1, keepdim=True), aterms.sum(1, keepdim=True)
    Ho = terms.shape[1]
    out = torch.zeros(n_rows, Ho, D, dtype=F64).index_add_(0, rows, aterms if absolute else terms)
    mag = torch.zeros(n_rows, Ho, D, dtype=F64).index_add_(0, rows, aterms)
    if o.addend is not None:
        a = o.addend.double()
        out, mag = out + (a.abs() if absolute else a), mag + a.abs()
        if mutant == 6:
            out[d.long_rows.cpu().long()] += a[d.long_rows.cpu().long()]
    if mutant == 2:
        out[int(out[:, Ho - 1, D - 1].abs().argmax()), Ho - 1, D - 1] = 0
    res = {"out": out, "terms": mag, "dot": None, "dterms": None, "mutant": mutant}
    if "dot" in c.entry:
        y = o.y.double()[rows]
        prod = xs * (y[:, None, :] if c.entry == "spmm_dot_bcast" else y)
        val, res["dterms"] = (prod.abs() if absolute else prod).sum(-1), torch.full((nnz, H), float("nan"), dtype=F64)
        res["dot"] = torch.full((nnz, H), float("nan"), dtype=F64)
        if getattr(o, "skip", False) and c.entry != "spmm_dot_bcast" and not absolute:
            # include/bot_gnn.h bot_spmm_set_zero_skip(1), the default: dot_out[wperm[k], h] = 0.f where w[wperm[k], h] is exactly 0
            val = torch.where(o.w.double()[AC._perm(o.wperm, nnz)] == 0, torch.zeros_like(val), val)
        at = torch.arange(nnz) if mutant == 7 else AC._perm(o.wperm, nnz)
        res["dot"][at] = val
        res["dterms"][at] = prod.abs().sum(-1)
    short = torch.ones(n_rows, dtype=torch.bool)
    if mutant == 9:
        short[d.long_rows.cpu().long()] = False
    m = out[short].float().abs()
    res["absmax"] = float(m.max()) if m.numel() else 0.0
    return res


# ------------------------------------------------------------------------------------------------ halves
def halves_encode(v32, s):
    """store_halves in numpy float32 / float16: z = v s, h1 = rn16(z), h2 = rn16((z - h1) 2048).  (h1, h2) as float16 arrays."""
    z = np.asarray(v32, dtype=np.float32) * np.float32(s)
    h1 = z.astype(np.float16)
    h2 = ((z - h1.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
    return h1, h2


def halves_layout(c, n_rows):
    """(ldh, hsh, h2_off, col0, width of a head's block) of the halves operand a case writes: a head's block is hpiece (bcast) or D
    columns, the head stride leaves a gap of 4 columns for H > 1 and the operand starts col0 = 8 columns into a wider row."""
    piece = c.hpiece if c.entry == "spmm_bcast_halves" else c.D
    hsh = (piece + 3) // 4 * 4 + 4
    h2_off = c.H * hsh
    return 8 + 2 * c.H * hsh + 8, hsh, h2_off, 8, piece


def halves_expected(o, ref_out, mutant=None):
    """The whole [n_rows, ldh] operand as int16 bit patterns: SENTINEL16 wherever the contract writes nothing, the halves of
    float32(ref_out) s, and zeros in the columns D .. hpiece - 1 of a head's block (bot_spmm_bcast_halves_f16 only)."""
    c = o.case
    ldh, hsh, h2_off, col0, piece = halves_layout(c, o.d.n_rows)
    buf = np.full((o.d.n_rows, ldh), SENTINEL16, dtype=np.int16)
    h1, h2 = halves_encode(ref_out.float().numpy(), float(o.hscale[0]))
    for h in range(c.H):
        c0 = col0 + h * hsh
        if c.entry == "spmm_bcast_halves" and mutant != 8:
            buf[:, c0 + c.D:c0 + piece] = 0
            buf[:, c0 + h2_off + c.D:c0 + h2_off + piece] = 0
        buf[:, c0:c0 + c.D] = h1[:, h].view(np.int16)
        buf[:, c0 + h2_off:c0 + h2_off + c.D] = h2[:, h].view(np.int16)
    return torch.from_numpy(buf)


def halves_decode(o, buf16):
    """(h1 + h2 / 2048) / s in float64 from the int16 bit patterns of an operand: [n_rows, H, D]."""
    c = o.case
    ldh, hsh, h2_off, col0, piece = halves_layout(c, o.d.n_rows)
    f = buf16.contiguous().view(torch.float16).double()
    out = torch.stack([f[:, col0 + h * hsh:col0 + h * hsh + c.D] + f[:, col0 + h * hsh + h2_off:col0 + h * hsh + h2_off + c.D] / 2048.0
                       for h in range(c.H)], 1)
    return out / float(o.hscale[0])


# ------------------------------------------------------------------------------------------------ bounds (module docstring)
def out_bound(o, ref):
    deg = AC.degrees(o.d).double()[:, None, None]
    h = o.case.H if o.case.entry == "spmm_dot_bcast" else 1
    return (deg * h + 2) * U * ref["terms"]


def dot_bound(o, ref):
    return (o.case.D + 1) * U * ref["dterms"]


def halves_bound(o, ref):
    b = out_bound(o, ref)
    return b + 2.0 ** -22 * (ref["out"].abs() + b) + 2.0 ** -36 / float(o.hscale[0])


def check(o, got, ref, exact, worst=None, tag=""):
    """Compare a result dict (CPU tensors: "out" [n_rows, Ho, D] or None, "dot" [nnz, H] or None, "halves" int16 [n_rows, ldh] or None,
    "absmax" float or None) with the restatement: bit for bit (exact) or entry for entry under the bounds.  Returns the list of
    differences found (empty: passed); worst: dict that keeps the largest error over its bound per output kind."""
    bad = []
    if got.get("out") is not None:
        want = ref["out"]
        if exact:
            ne = got["out"].contiguous().view(torch.int32) != want.float().view(torch.int32)
            if bool(ne.any()):
                at = ne.nonzero()
                bad.append("out: %d differ, first (index, got, want) %s" % (
                    at.shape[0], [(tuple(t.tolist()), float(got["out"][tuple(t)]), float(want[tuple(t)])) for t in at[:4]]))
        else:
            _under(bad, worst, "out" + tag, (got["out"].double() - want).abs(), out_bound(o, ref))
    if got.get("dot") is not None and ref["dot"] is not None:
        want, written = ref["dot"], ~torch.isnan(ref["dot"])
        g = got["dot"]
        if not torch.equal(g.view(torch.int32)[~written], torch.full_like(g.view(torch.int32)[~written], SENTINEL32)):
            bad.append("dot written where nothing belongs")
        if exact:
            if not torch.equal(g[written].view(torch.int32), want[written].float().view(torch.int32)):
                bad.append("dot")
        else:
            _under(bad, worst, "dot" + tag, (g.double() - want).abs()[written], dot_bound(o, ref)[written])
    if got.get("halves") is not None:
        want = halves_expected(o, ref["out"], ref["mutant"])
        if exact:
            if not torch.equal(got["halves"], want):
                at = (got["halves"] != want).nonzero()
                bad.append("halves: %d differ, first (row, column, got, want) %s" % (
                    at.shape[0], [(int(r), int(k), int(got["halves"][r, k]), int(want[r, k])) for r, k in at[:4]]))
        else:
            pad = _padding_mask(o)
            if not torch.equal(got["halves"][pad], want[pad]):
                bad.append("halves padding / guards")
            _under(bad, worst, "halves" + tag, (halves_decode(o, got["halves"]) - ref["out"]).abs(), halves_bound(o, ref))
    if got.get("absmax") is not None:
        # exactly max |out| of what the call itself wrote, which is the restatement's in the exact regime and within the largest `out`
        # bound of it otherwise
        own = float(got["out"].abs().max()) if got["out"].numel() else 0.0
        if got["absmax"] != own or (got["absmax"] != ref["absmax"] if exact else
                                    abs(got["absmax"] - ref["absmax"]) > float(out_bound(o, ref).max())):
            bad.append("absmax")
    return bad


def _padding_mask(o):
    """True where the halves operand holds no value: guards (sentinel) and zero padding."""
    c = o.case
    ldh, hsh, h2_off, col0, piece = halves_layout(c, o.d.n_rows)
    m = torch.ones(o.d.n_rows, ldh, dtype=torch.bool)
    for h in range(c.H):
        for base in (col0 + h * hsh, col0 + h * hsh + h2_off):
            m[:, base:base + c.D] = False
    return m


def _under(bad, worst, name, err, bound):
    if err.numel() == 0:
        return
    if bool(torch.isnan(err).any()) or bool((err > bound).any()):
        bad.append(name)
    if worst is not None:
        ratio = float((err / bound.clamp(min=1e-300)).max())
        worst[name] = max(worst.get(name, 0.0), ratio)


# ------------------------------------------------------------------------------------------------ placement
def place(t, r, device, contiguous=False):
    """A view holding the input t ([n, H, D] or [n, D]) inside one larger allocation on `device` under recipe r, with GUARD floats before
    and after; padding columns and guards hold NaN.  contiguous: an [H, n, D] operand that is contiguous by contract (bot_spmm_dot_bcast's
    x), only the base offset applies.  Returns (buffer, view)."""
    buf, view = _place(tuple(t.shape), r, device, contiguous, float("nan"))
    view.copy_(t.to(device))
    return buf, view


def place_out(shape, r, device):
    """The same for an output of `shape`: every word, the view's own included, holds SENTINEL32 (guards_intact, and a result entry that
    is never written shows)."""
    return _place(tuple(shape), r, device, False, None)


def _place(shape, r, device, contiguous, fill):
    if len(shape) == 3 and not contiguous:
        n, Hh, Dd = shape
        ld, hs = strides(Hh, Dd, r)
        if Hh == 1:
            hs = Dd
        size, st = n * ld, (ld, hs, 1)
    elif len(shape) == 2:
        n, Dd = shape
        ld = Dd + r.pad
        size, st = n * ld, (ld, 1)
    else:                                                   # contiguous [H, n, D]
        size, st = shape[0] * shape[1] * shape[2], (shape[1] * shape[2], shape[2], 1)
    buf = torch.empty(GUARD + r.off + size + GUARD + 4, dtype=torch.float32, device=device)
    if fill is None:
        buf.view(torch.int32).fill_(SENTINEL32)
    else:
        buf.fill_(fill)
    return buf, torch.as_strided(buf, shape, st, GUARD + r.off)


def guards_intact(buf, view, r):
    """Every word of an output's allocation outside the view still holds SENTINEL32."""
    mask = torch.ones_like(buf, dtype=torch.bool)
    torch.as_strided(mask, view.shape, view.stride(), GUARD + r.off).fill_(False)
    return bool((buf.view(torch.int32)[mask] == SENTINEL32).all())
