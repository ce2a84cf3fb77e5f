"""Float64 restatements of the node-axis BatchNorm + ReLU + dropout passes (csrc/dense.hip; include/bot_gnn.h bot_colstats_f32,
bot_colsum_f32, bot_bn_stats_f32, bot_bn_stats_halves_f32, bot_bn_stats_halves_partials_f32, bot_bn_act_fwd_f32 / _halves_f32,
bot_bn_act_bwd_reduce_f32 / _max_f32, bot_bn_bwd_bound_f32, bot_bn_act_bwd_apply_f32 / _halves_f32 and the second stages over partials a
GEMM delivered), shared by tests/test_bn_host.py and tests/test_bn_gpu.py: the contract in plain torch float64 FROM THE FLOAT32 OPERANDS
EACH KERNEL IS GIVEN (mean and invstd are the vectors handed in, never recomputed), the Philox dropout mask, the halves layouts, a Python
restatement of the dispatch (which launch form a call records with set_kernel) with the names counted from it, the covering case list
with its coverage ASSERTED from its own enumeration, the exact regime with its premises asserted, the bounds for seeded inputs and the
mutants of the restatement that show the checks are not vacuous.  Nothing here calls the code under test.

The contract.  keep(r, c) = ((word c % 4 of Philox4x32-10(key, counter r * ceil(F / 4) + c // 4)) >> 8) * 2^-24 >= float32(p), key =
seed + seed_offset * 0x9E3779B97F4A7C15 (AC.drop_seed), factor f = float32(1 / (1 - p)).  With t = (x - mean) invstd w and pre = t + b:
    y = relu?(pre) keep f;  g = dy keep f [pre > 0];  xhat = (x - mean) invstd;  sum_g = sum_r g;  sum_gx = sum_r g xhat;
    dx = w invstd (g - sum_g c - xhat sum_gx c),  c = float32(1 / total_count)  (sum_g None, eval statistics: dx = w invstd g).

The dispatch (`bn_form`).  pick_vec gives 4 / 2 / 1 from F, the row pitches and the base addresses; bn_vec turns "even F, even pitches,
8-byte bases" into the quad form: VEC = 4 lanes whose operands move as float4 where base and pitch are 16-byte multiples (`wide`) and as
two float2 elsewhere.  `bn_vec` can NEVER return 2: pick_vec returns 2 exactly when F and every pitch are even and every base is 8-byte
aligned (and 4 was not possible), and those are the quad conditions, so the call leaves as (4, quad).  `unreachable_vec2()` confirms it by
enumeration; the <2> instantiations of the five templates are dead code.

Exact regime.  x, mean, b, dy, sum_g, sum_gx integers, invstd and |w| powers of two, p in {0, 0.5, 0.75} (f = 1, 2, 4), total_count a
power of two: every intermediate of every expression above is a float32 number (`assert_exact` checks each one), so forward, gate, apply
and both halves are bit-exact whatever the compiler contracts; column sums of multiples of 0.25 whose absolute terms stay below
EXACT_LIMIT are exact in every order, so sum_g, sum_gx, colsum and the column maxima are too.  Statistics: integer columns have integer
pivots, S and Q are exact; where n is a power of two S / n and Q - S^2 / n are exact in double and mean / M2 are the single rounding of
the float64 value.

Bounds for seeded inputs (U = 2^-24, gamma_k = k U / (1 - k U)), entry for entry, from lengths and magnitudes of the restatement only;
one rounding per written operation (a contracted a * b + c only removes one):
- pre: the subtraction, invstd * w and the fmaf: E_pre = gamma_3 (|t| + |b|); y: one more product by f: E_y = gamma_4 f (|t| + |b|)
  (|relu a - relu b| <= |a - b|: the gate needs no policy in the forward values).
- an entry is UNDECIDED where |pre| <= E_pre (the backward's expression has three roundings too): element-wise checks accept either
  gate there and the sums' bounds widen by its |g| and |g xhat|.  At most 1e-4 of a case's entries may be undecided (host test).
- two-stage sums: a thread adds R = ceil(n / (4 nblk)) rows, nblk = min(ceil(n / 4), 256), the workgroup adds kTY = 4 of those, the
  second stage adds the nblk partials in double (2^-53 per addition, inside the + 1) and rounds once:
  (R + kTY + 2 + k + 1) U sum |term|, k = the roundings of a term: 1 for g (the product by f), 4 for g xhat (+ the subtraction, the
  product by invstd and the fmaf's own).  Column maxima: gamma_1 max |g| and gamma_2 max |xhat|.
- dx: on the longest path xhat (2), sum_gx c (1), their product (1), the subtraction (1), w invstd (1) and the last product (1):
  E_dx = gamma_7 |w| invstd (|g| + |sum_g c| + |xhat sum_gx c|).
- statistics (pivot = the column's first row, d = x - pivot): S = sum d, Q = sum d^2; e_S = (R + kTY + 4) U sum |d|, e_Q = (R + kTY + 6) U
  sum d^2; mean = pivot + S / n: e_S / n + U |mean|; M2 = Q - S^2 / n: e_Q + (2 |S| e_S + e_S^2) / n + U M2.  Both hold with the pivot's
  own sums, not the centred ones: a far pivot widens them, as it widens the error.  invstd = rsqrtf(M2 / n + eps): the argument's
  relative error is (e_M2 / n + 3 U a) / a (division taken as 2 U, the addition 1 U) and the result's half of it + RSQRT_ERR.
- running statistics: gamma_4 (|rm (1 - m)| + |m mean|) + m e_mean and gamma_6 (|rv (1 - m)| + |m M2 / (n - 1)|) + m e_M2 / (n - 1).
- decoded halves: SC's bound, B + 2^-22 (|ref| + B) + 2^-36 / s."""
import collections
import functools
import itertools
import types

import numpy as np
import torch

from tests import _oracle_backend as OB
from tests import attn_cases as AC
from tests import spmm_cases as SC
from tests.test_sampling_host import philox4x32_10

F64 = torch.float64
U, EXACT_LIMIT = AC.U, AC.EXACT_LIMIT
Recipe = SC.Recipe
kTX, kTY, kRowBlocks, kRowSeg = 64, 4, 256, 8
# rsqrtf against float64, measured on the MI355X through bot_bn_stats_f32 itself (tests/test_bn_gpu.py
# test_rsqrt_error_measured_fp64): two-row columns (+a, -a), eps = 0, whose variance a^2 is a float32 number, 4 096 seeded a.
RSQRT_MEASURED = 7.8697e-08       # 1.320 U, at the argument 2.60770073e+17 (below the 4 U above which it would be a finding)
RSQRT_ERR = 2 * RSQRT_MEASURED
UNDECIDED_SHARE = 1e-4


def gamma(k):
    return k * U / (1 - k * U)


# ------------------------------------------------------------------------------------------------ the dispatch, restated
def bn_form(F, strides, byte_offsets):
    """csrc/dense.hip bn_vec + rows16 -> (vec, quad, wide flag per operand).  byte_offsets: each operand's base address mod 16, None
    for an absent operand (a NULL pointer constrains nothing and is never wide)."""
    present = [b for b in byte_offsets if b is not None]
    v = SC.vec_of(F, strides, present)
    wide = tuple(b is not None and b % 16 == 0 and s % 4 == 0 for s, b in zip(strides, byte_offsets))
    if v == 4 or F % 2 or any(s % 2 for s in strides) or any(b % 8 for b in present):
        return v, False, wide
    return 4, True, wide


def _name(kernel, vec, quad, extra, flags):
    s = "bot::%s<%d>%s" % (kernel, vec, extra)
    if quad:
        s += " quad" + "".join(" %s=%d" % (k, int(v)) for k, v in flags)
    return s


def partial_name(F, ldx, bx):
    v, q, (wx,) = bn_form(F, (ldx,), (bx,))
    return _name("colstats_partial_kernel", v, q, "", (("wx", wx),))


def piece_of(F):
    return (F + 63) // 64 * 64


def fwd_form(F, ldx, bx, ldy, by, pieces=0, piece=None):
    """-> (name, vec, "plain" / "rowseg" / "tiled").  by None: no fp32 output (its pitch then counts as ldx)."""
    if by is None:
        ldy = ldx
    v, q, (wx, wy) = bn_form(F, (ldx, ldy), (bx, by))
    flags = (("wx", wx), ("wy", wy))
    if not pieces:
        return _name("bn_act_fwd_kernel", v, q, "", flags), v, "plain"
    assert v == 4, "the halves forward needs the 4-column form"
    piece = piece_of(F) if piece is None else piece
    if piece <= 1024:
        return _name("bn_act_fwd_rowseg_kernel", 4, q, " rowseg pieces=%d" % pieces, flags), 4, "rowseg"
    return _name("bn_act_fwd_kernel", 4, q, " tiled pieces=%d" % pieces, flags), 4, "tiled"


def reduce_name(F, ldx, bx, lddy, bdy):
    v, q, (wx, wdy) = bn_form(F, (ldx, lddy), (bx, bdy))
    return _name("bn_act_bwd_reduce_kernel", v, q, "", (("wx", wx), ("wdy", wdy)))


def apply_name(F, ldx, bx, lddy, bdy, lddx, bdx, halves=False):
    if bdx is None:
        lddx = ldx
    v, q, (wx, wdy, wdx) = bn_form(F, (ldx, lddy, lddx), (bx, bdy, bdx))
    return _name("bn_act_bwd_apply_kernel", v, q, " halves" if halves else "", (("wx", wx), ("wdy", wdy), ("wdx", wdx)))


SECOND_STAGES = ("bot::bn_bwd_bound_kernel", "bot::pair_final_wide_kernel", "bot::bn_bwd_bound_wide_kernel", "bot::bn_bwd_finish_wide_kernel",
                 "bot::colstats_tiles_final_kernel")
_GRID = [(off, pad) for off in (0, 1, 2) for pad in (0, 1, 2, 4, 6)]


@functools.lru_cache(maxsize=None)
def all_forms():
    """Every name the restated dispatch can produce, by enumeration over widths, base offsets and pitches."""
    names = set(SECOND_STAGES)
    for F in (5, 6, 8, 1026, 1028):
        ops = [(F + pad, 4 * off) for off, pad in _GRID]
        for ldx, bx in ops:
            names.add(partial_name(F, ldx, bx))
            for ld2, b2 in ops:
                names.add(fwd_form(F, ldx, bx, ld2, b2)[0])
                names.add(reduce_name(F, ldx, bx, ld2, b2))
                if bn_form(F, (ldx, ld2), (bx, b2))[0] == 4:
                    for pieces in (2, 3):
                        names.add(fwd_form(F, ldx, bx, ld2, b2, pieces)[0])
                for ld3, b3 in ops:
                    for h in ((False, True) if F % 2 == 0 else (False,)):
                        names.add(apply_name(F, ldx, bx, ld2, b2, ld3, b3, h))
    return frozenset(names)


N_FORMS = 61     # 4 partial, 6 forward, 10 row-segment, 10 column-tiled halves forward, 6 reduce, 10 + 10 apply, 5 second stages


def unreachable_vec2():
    """True iff no (F, pitches, bases) of the enumeration leaves bn_form with vec 2 (module docstring)."""
    for F in range(1, 13):
        for k in (1, 2, 3):
            for ops in itertools.product(_GRID, repeat=k):
                if bn_form(F, [F + pad for _, pad in ops], [4 * off for off, _ in ops])[0] == 2:
                    return False
    return True


def nblk_of(n):
    return min(max((n + kTY - 1) // kTY, 1), kRowBlocks)


def rows_per_thread(n):
    return -(-n // (kTY * nblk_of(n)))


# ------------------------------------------------------------------------------------------------ the case list
Case = collections.namedtuple("Case", "n F rx rdy rdx ry relu affine p off regime max evalmode hd tag")
"""One chain of calls on an [n, F] operand: the statistics, the forward (plain and, where the form allows, the halves at both piece
counts and without y), the reduce pass (max: with the column maxima and bn_bwd_bound), the apply pass (absmax always; evalmode: sum_g
None) and, hd = (hD, hDP), the apply pass writing halves.  r*: SC.Recipe of x, dy, dx, y; affine: which of weight / bias exist; off: the
seed offset word or None."""
ROWS = (1, 2, 3, 4, 5, 7, 8, 9, 1023, 1024, 1025, 2049, 4095, 4096, 4097, 5121, 8193)
NBLK = (1, 2, 3, 4, 5, 28, 29, 32, 33, 61, 255, 256)
NBLK_ROWS = (3, 6, 11, 13, 19, 111, 115, 127, 131, 243, 1019, 1021)     # ragged n with ceil(n / 4) = the values of NBLK
COLS = (1, 2, 3, 4, 5, 6, 63, 64, 65, 254, 255, 256, 257, 258, 750, 960, 962, 1024, 1026, 1030)
PLACE_F = (6, 8, 258, 750, 1026, 1028)       # 1026 / 1028: the column-tiled halves forward at every quad flag combination too
PLACE_N = 37
PS = (0.0, 0.5, 0.75, 0.3)
AFFINE = ("wb", "w", "b", None)
HEADS = ((2, 2), (6, 8), (250, 256), (64, 64))
STAGE_NBLK_WIDE = (1, 15, 16, 17, 48, 49, 64, 65, 112, 113, 128, 129, 241, 300)
STAGE_NBLK_TILES = (1, 2, 63, 64, 65, 192, 193, 256, 257, 300)
STAGE_LAST = (1, 255, 256)
STAGE_F = (1, 15, 16, 17, 31, 32, 33, 40)
R0 = Recipe()


def _wide(F, i=0):
    """A recipe whose rows are 16-byte aligned: pitch a multiple of 4."""
    return Recipe(pad=((-F) % 4) + 4 * (i % 2))


def _narrow(F, i=0):
    """8-byte rows that are not 16-byte rows: a base 8 bytes in, or a pitch 2 mod 4."""
    return Recipe(off=2, pad=(F % 2) * 0) if i % 2 == 0 else Recipe(pad=(2 - F % 4) % 4)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    k = 0

    def add(n, F, tag, regime=None, **kw):
        nonlocal k
        p = kw.pop("p", PS[k % 4])
        reg = regime or ("exact" if (k % 2 == 0 and p != 0.3) else "seeded")
        if reg == "exact" and p == 0.3:
            p = 0.5
        c = dict(rx=R0, rdy=R0, rdx=R0, ry=R0, relu=k % 3 != 2, affine=AFFINE[(k // 2) % 4], p=p, off=(None if k % 3 else 1 + k % 5), regime=reg,
                 max=k % 2 == 0, evalmode=k % 5 == 3, hd=None, tag=tag)
        c.update(kw)
        out.append(Case(n=n, F=F, **c))
        k += 1

    # rows x columns: every n against a narrow F, every F against a small n, and the wide F against the rows that turn the unroll
    small_f = (5, 6, 8, 3, 258, 64, 65, 4)
    for i, n in enumerate(ROWS + NBLK_ROWS):
        add(n, small_f[i % len(small_f)] if n > 2049 else COLS[(3 * i + 5) % len(COLS)], "rows")
    small_n = (9, 37, 5, 130, 21)
    for i, F in enumerate(COLS):
        add(small_n[i % len(small_n)], F, "cols")
        add(small_n[(i + 2) % len(small_n)] + 1, F, "cols", regime="seeded", p=PS[(i + 1) % 4])
    for n, F in ((1025, 1026), (4097, 962), (2049, 1030), (4097, 258), (1025, 750)):
        add(n, F, "big", regime="exact", p=0.5)
        add(n, F, "big", regime="seeded", p=0.3)
    # placement: every operand independently wide / narrow (all 16 combinations per F), and 4-byte placements
    for F in PLACE_F:
        for i, (a, b, c_, d) in enumerate(itertools.product((0, 1), repeat=4)):
            rs = [(_wide(F, i + j) if bit == 0 else _narrow(F, i + j)) for j, bit in enumerate((a, b, c_, d))]
            add(PLACE_N, F, "place", rx=rs[0], rdy=rs[1], rdx=rs[2], ry=rs[3], hd=(2, 2) if i % 2 else None)
        add(PLACE_N, F, "place", rx=Recipe(off=1), hd=(2, 2))
        add(PLACE_N, F, "place", rdy=Recipe(pad=1), ry=Recipe(off=1), regime="seeded", p=0.3)
        add(PLACE_N, F, "place", rdx=Recipe(off=1, pad=1), ry=Recipe(pad=1), regime="exact", p=0.75)
    # the apply pass writing halves: head blocks of hD every hDP
    for i, (hD, hDP) in enumerate(HEADS):
        for j, (rx, rdy) in enumerate(((R0, R0), (Recipe(off=2), R0), (Recipe(off=1), R0), (_wide(3 * hD), _narrow(3 * hD, 1)))):
            add((37, 9, 130, 6)[j], 3 * hD, "heads", rx=rx, rdy=rdy, hd=(hD, hDP), regime=("exact", "seeded")[(i + j) % 2], p=PS[(i + j) % 4])
    return tuple(out)


def vecs_of(c):
    """(byte offset, pitch) of the four operands of a case."""
    return {k: (4 * r.off, c.F + r.pad) for k, r in (("x", c.rx), ("dy", c.rdy), ("dx", c.rdx), ("y", c.ry))}


def halves_fwd_ok(c):
    o = vecs_of(c)
    return bn_form(c.F, (o["x"][1], o["y"][1]), (o["x"][0], o["y"][0]))[0] == 4 and bn_form(c.F, (o["x"][1],), (o["x"][0],))[0] == 4


def expected_names(c):
    """kind -> name of every launch form the chain of case c records."""
    o = vecs_of(c)
    (bx, ldx), (bdy, lddy), (bdx, lddx), (by, ldy) = o["x"], o["dy"], o["dx"], o["y"]
    names = {"partial": partial_name(c.F, ldx, bx), "fwd": fwd_form(c.F, ldx, bx, ldy, by)[0], "reduce": reduce_name(c.F, ldx, bx, lddy, bdy),
             "apply": apply_name(c.F, ldx, bx, lddy, bdy, lddx, bdx)}
    if halves_fwd_ok(c):
        for pieces in (2, 3):
            names["fwd_h%d" % pieces] = fwd_form(c.F, ldx, bx, ldy, by, pieces)[0]
        names["fwd_h_only"] = fwd_form(c.F, ldx, bx, ldx, None, 2)[0]
    if c.hd:
        names["apply_h"] = apply_name(c.F, ldx, bx, lddy, bdy, lddx, bdx, True)
        names["apply_h_only"] = apply_name(c.F, ldx, bx, lddy, bdy, ldx, None, True)
    if c.max:
        names["bound"] = SECOND_STAGES[0]
    return names


def stage_cases():
    """(kind, nblk, F, last-block rows) of the second stages fed with synthetic partials."""
    out = []
    for i, nblk in enumerate(STAGE_NBLK_WIDE):
        out.append(("wide", nblk, STAGE_F[i % len(STAGE_F)], 256))
        out.append(("wide", nblk, STAGE_F[(i + 3) % len(STAGE_F)], 256))
    for i, nblk in enumerate(STAGE_NBLK_TILES):
        for j, last in enumerate(STAGE_LAST):
            out.append(("tiles", nblk, STAGE_F[(i + 3 * j) % len(STAGE_F)], last))
    return out


def assert_coverage():
    """Every value the case list promises is reached, counted from the list itself."""
    cs = cases()
    ns, Fs = {c.n for c in cs}, {c.F for c in cs}
    assert set(ROWS) <= ns and set(NBLK_ROWS) <= ns and set(COLS) <= Fs and set(PLACE_F) <= Fs
    assert {nblk_of(n) for n in NBLK_ROWS} == set(NBLK) and {nblk_of(n) for n in ns} >= set(NBLK)
    assert {rows_per_thread(n) for n in ns} >= {1, 2, 4, 5, 6, 9}       # the UR = 4 unroll: under one trip, a full one, a second
    for regime in ("exact", "seeded"):
        sub = [c for c in cs if c.regime == regime]
        assert {c.relu for c in sub} == {True, False} and {c.affine for c in sub} == set(AFFINE)
        assert {c.p for c in sub} >= ({0.0, 0.5, 0.75} if regime == "exact" else set(PS))
        assert {c.off is None for c in sub} == {True, False} and {c.max for c in sub} == {True, False} and {c.evalmode for c in sub} == {True, False}
        assert {c.hd for c in sub} >= set(HEADS)
    assert all(c.p in (0.0, 0.5, 0.75) for c in cs if c.regime == "exact")
    names = set(SECOND_STAGES)
    for c in cs:
        names |= set(expected_names(c).values())
    assert names == all_forms(), sorted(all_forms() ^ names)
    assert len(all_forms()) == N_FORMS, len(all_forms())
    # what no earlier test launched: the column-tiled halves forward, vec 1 with halves in the apply, every quad flag combination
    assert any("tiled" in s for s in names) and "bot::bn_act_bwd_apply_kernel<1> halves" in names
    assert {fwd_form(c.F, *_xy(c), 3)[2] for c in cs if halves_fwd_ok(c)} == {"rowseg", "tiled"}
    assert any(piece_of(c.F) == 1088 for c in cs) and any(piece_of(c.F) == 1024 and c.F > 960 for c in cs)
    st = stage_cases()
    assert {s[1] for s in st if s[0] == "wide"} == set(STAGE_NBLK_WIDE) and {s[1] for s in st if s[0] == "tiles"} == set(STAGE_NBLK_TILES)
    assert {s[2] for s in st} == set(STAGE_F) and {(s[1], s[3]) for s in st if s[0] == "tiles"} == set(itertools.product(STAGE_NBLK_TILES, STAGE_LAST))
    return len(cs), len(st)


def _xy(c):
    o = vecs_of(c)
    return o["x"][1], o["x"][0], o["y"][1], o["y"][0]


# ------------------------------------------------------------------------------------------------ the dropout mask, restated
def keep_mask(n, F, p, seed, seed_offset=None, mutant=None):
    """bool [n, F]: element (r, c) takes word c % 4 of the Philox block with counter r * ceil(F / 4) + c // 4 and is kept iff
    float32((w >> 8) * 2^-24) >= float32(p)."""
    if p <= 0:
        return torch.ones(n, F, dtype=torch.bool)
    nq = (F + 3) // 4
    rows = np.arange(n, dtype=np.uint64)[:, None] * np.uint64(1 if mutant == 1 else nq)       # mutant 1: the counter without ceil(F / 4)
    ctr = (rows + np.arange(nq, dtype=np.uint64)[None, :]).reshape(-1)
    w = philox4x32_10(AC.drop_seed(seed, seed_offset), ctr).reshape(n, nq, 4)
    if mutant == 2:                                                                            # the word of a 2-wide lane (c % 2) instead of c % 4
        w = w[:, :, [0, 1, 0, 1]]
    w = w.reshape(n, nq * 4)[:, :F]
    u = ((w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
    return torch.from_numpy(u >= np.float32(p))


def drop_factor(p):
    return AC.drop_scale(p) if p > 0 else 1.0


# ------------------------------------------------------------------------------------------------ inputs
MUTANTS = {1: "the mask counter without ceil(F / 4)", 2: "word c % 4 replaced by the lane's element index", 3: "n for n - 1 in the running variance",
           4: "the gate on >= 0", 5: "sum_gx without xhat", 6: "a dropped last row", 7: "a dropped last column pair",
           8: "the second half not shifted by 2^11", 9: "head blocks at hD instead of hDP"}


def _f(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float32))


def make_inputs(c, seed):
    """The float32 operands of a case (CPU): x, dy [n, F]; mean, invstd, w, b, sum_g, sum_gx [F]; the dropout key; total_count."""
    rng = np.random.default_rng(seed)
    n, F = c.n, c.F
    i = types.SimpleNamespace(case=c, seed=1234567 + 1000 * seed, off=c.off, eps=1e-5, momentum=0.1)
    if c.regime == "exact":
        i.mean = _f(rng.integers(-3, 4, F))
        i.x = _f(rng.integers(-5, 6, (n, F))) + i.mean
        i.invstd = _f(2.0 ** rng.integers(-2, 1, F))
        i.w = _f(2.0 ** rng.integers(-1, 2, F) * rng.choice([-1.0, 1.0], F))
        i.b = _f(rng.integers(-2, 3, F))
        i.dy = _f(rng.integers(-2, 3, (n, F)))
        i.total_count = 1024.0
        i.sum_g, i.sum_gx = _f(rng.integers(-64, 65, F)), _f(rng.integers(-64, 65, F))
    else:
        spread, centre = _f(np.exp(rng.normal(0, 0.7, F))), _f(rng.normal(0, 2.0, F))
        i.x = _f(rng.normal(0, 1, (n, F))) * spread + centre
        X = i.x.double()
        i.mean = X.mean(0).float()
        i.invstd = (1.0 / torch.sqrt(X.var(0, unbiased=False) + 1e-5)).float() if n > 1 else _f(np.full(F, 316.0))
        i.w, i.b = _f(rng.normal(0, 1, F) + 0.25), _f(rng.normal(0, 0.3, F) + 0.1)
        i.dy = _f(rng.normal(0, 1, (n, F)))
        i.total_count = float(n)
        i.sum_g = i.sum_gx = None       # filled from the restated reduce pass below
    if c.affine in ("b", None):
        i.w = None
    if c.affine in ("w", None):
        i.b = None
    i.rm, i.rv = _f(rng.integers(-2, 3, F)), _f(rng.integers(1, 4, F))
    if i.sum_g is None:
        r = reference(i, want_dx=False)
        i.sum_g, i.sum_gx = r["sum_g"].float(), r["sum_gx"].float()
    return i


def assert_exact(i, r):
    """The premises of the exact regime: every intermediate of the restatement is a float32 number (so no rounding happens anywhere,
    contracted or not) and the sums stay below EXACT_LIMIT in multiples of 0.25."""
    for k in ("d", "sw", "t", "pre", "y", "xhat", "g", "gx", "mg", "mgx", "xmgx", "g_mg", "inner", "wis", "dx", "dx_eval"):
        v = r[k]
        assert torch.equal(v.float().double(), v), k
    for k in ("g", "gx"):
        assert torch.equal((r[k] * 4).round(), r[k] * 4) and float(r[k].abs().sum(0).max()) < EXACT_LIMIT, k
    assert float(i.x.abs().sum(0).max()) < EXACT_LIMIT and float(np.log2(i.total_count)).is_integer()
    assert float(np.float32(drop_factor(i.case.p))) in (1.0, 2.0, 4.0)


# ------------------------------------------------------------------------------------------------ the contract in float64
def reference(i, mutant=None, want_dx=True):
    c = i.case
    n, F = c.n, c.F
    x, dy, mean, invstd = i.x.double(), i.dy.double(), i.mean.double(), i.invstd.double()
    w = i.w.double() if i.w is not None else torch.ones(F, dtype=F64)
    b = i.b.double() if i.b is not None else torch.zeros(F, dtype=F64)
    f = drop_factor(c.p)
    keep = keep_mask(n, F, c.p, i.seed, i.off, mutant)
    r = {"mutant": mutant, "keep": keep}
    r["d"] = x - mean
    r["sw"] = invstd * w
    r["t"] = r["d"] * r["sw"]
    r["pre"] = r["t"] + b
    r["e_pre"] = gamma(3) * (r["t"].abs() + b.abs())
    # (pre_slack: what the statistics' own error moves pre by, where a composed call forms them itself)
    r["und"] = (r["pre"].abs() <= r["e_pre"] + getattr(i, "pre_slack", 0.0)) if (c.relu and c.regime == "seeded") else torch.zeros(n, F, dtype=torch.bool)
    gate = ((r["pre"] >= 0) if mutant == 4 else (r["pre"] > 0)) if c.relu else torch.ones(n, F, dtype=torch.bool)
    kf = keep.double() * f
    r["y"] = (torch.relu(r["pre"]) if c.relu else r["pre"]) * kf
    r["e_y"] = gamma(4) * f * (r["t"].abs() + b.abs())
    r["xhat"] = r["d"] * invstd
    r["g"] = dy * kf * gate
    r["g_alt"] = dy * kf * (gate ^ r["und"])                 # the other gate where undecided
    r["gx"] = r["g"] if mutant == 5 else r["g"] * r["xhat"]
    rows = slice(0, n - 1) if mutant == 6 else slice(0, n)
    r["sum_g"], r["sum_gx"] = r["g"][rows].sum(0), r["gx"][rows].sum(0)
    R = rows_per_thread(n) + kTY + 3
    wid_g, wid_gx = (r["g"] - r["g_alt"]).abs().sum(0), ((r["g"] - r["g_alt"]) * r["xhat"]).abs().sum(0)
    r["e_sum_g"] = (R + 1) * U * r["g"].abs().sum(0) + wid_g * (1 + (R + 1) * U)
    r["e_sum_gx"] = (R + 4) * U * (r["g"] * r["xhat"]).abs().sum(0) + wid_gx * (1 + (R + 4) * U)
    r["gmax"], r["xmax"] = r["g"].abs().max(0).values, r["xhat"].abs().max(0).values
    r["gmax_alt"] = torch.maximum(r["g"].abs(), r["g_alt"].abs()).max(0).values
    if not want_dx:
        return r
    cinv = getattr(i, "cinv", float(np.float32(1.0 / i.total_count)))      # (the kernel is handed float32(1 / total_count))
    sg, sgx = i.sum_g.double(), i.sum_gx.double()
    r["mg"], r["mgx"] = sg * cinv, sgx * cinv
    r["xmgx"] = r["xhat"] * r["mgx"]
    r["g_mg"] = r["g"] - r["mg"]
    r["inner"] = r["g_mg"] - r["xmgx"]
    r["wis"] = w * invstd
    r["dx"] = r["wis"] * r["inner"]
    r["dx_alt"] = r["wis"] * (r["g_alt"] - r["mg"] - r["xmgx"])
    r["e_dx"] = gamma(7) * r["wis"].abs() * (r["g"].abs() + r["g_alt"].abs() + r["mg"].abs() + r["xmgx"].abs())
    r["dx_eval"] = r["wis"] * r["g"]
    r["dx_eval_alt"] = r["wis"] * r["g_alt"]
    r["e_dx_eval"] = gamma(3) * r["wis"].abs() * torch.maximum(r["g"].abs(), r["g_alt"].abs())
    if mutant == 7 and F >= 2:                                # the last column pair never written: whatever the output held before
        for k in ("y", "dx", "dx_eval"):
            r[k] = r[k].clone()
            r[k][:, F - 2:] = float("nan")
    return r


def undecided_share(i, r):
    return float(r["und"].double().mean())


def bwd_bound64(i, r, evalmode):
    """bn_bwd_bound_kernel's formula in float64 from the restated column maxima and the sums handed in: (value, with the other gate's
    maxima where an entry is undecided)."""
    w = i.w.double().abs() if i.w is not None else 1.0
    cinv = float(np.float32(1.0 / i.total_count))

    def form(gm):
        t = gm if evalmode else gm + i.sum_g.double().abs() * cinv + r["xmax"] * i.sum_gx.double().abs() * cinv
        return float((w * i.invstd.double() * t).max())
    return form(r["gmax"]), form(r["gmax_alt"])


# ------------------------------------------------------------------------------------------------ statistics
def stats64(x, eps, momentum, rm=None, rv=None, nbt=None, mutant=None):
    """mean, M2, invstd, the running statistics after the step (unbiased variance, n > 1 ? n - 1 : 1) and the step counter, with the
    bounds of the module docstring."""
    X = x.double()
    n = X.shape[0]
    eps, momentum = float(np.float32(eps)), float(np.float32(momentum))
    mean = X.mean(0)
    m2 = ((X - mean) ** 2).sum(0)
    d = X - X[0]
    S, sabs, Q = d.sum(0), d.abs().sum(0), (d * d).sum(0)
    R = rows_per_thread(n) + kTY
    e_S, e_Q = (R + 4) * U * sabs, (R + 6) * U * Q + n * 2.0 ** -126        # (squares below the normal range: absolutely)
    r = {"mean": mean, "m2": m2, "sum": X.sum(0), "e_sum": (R + 3) * U * X.abs().sum(0)}
    r["e_mean"] = e_S / n + U * mean.abs()
    r["e_m2"] = e_Q + (2 * S.abs() * e_S + e_S * e_S) / n + U * m2
    a = m2 / n + eps
    r["invstd"] = 1.0 / torch.sqrt(a)
    rel = (r["e_m2"] / n + 3 * U * a) / a
    r["e_invstd"] = r["invstd"] * (0.5 * rel / (1 - rel).clamp(min=0.5) + rel * rel + RSQRT_ERR)
    if rm is not None:
        den = n if mutant == 3 else (n - 1 if n > 1 else 1)
        r["rm"] = rm.double() * (1 - momentum) + momentum * mean
        r["rv"] = rv.double() * (1 - momentum) + momentum * m2 / den
        r["e_rm"] = gamma(4) * ((rm.double() * (1 - momentum)).abs() + (momentum * mean).abs()) + momentum * r["e_mean"]
        r["e_rv"] = gamma(6) * ((rv.double() * (1 - momentum)).abs() + momentum * m2 / den) + momentum * r["e_m2"] / den
    r["nbt"] = None if nbt is None else int(nbt) + 1
    return r


def bound64(x, mean, invstd, w, b, p):
    """The epilogue bound (|w| max(|max - mean|, |min - mean|) invstd + |b|) / (1 - p) per column from the float32 statistics handed
    in, and the power-of-two scale from its maximum (OB._pow2_scale)."""
    X = x.double()
    dev = torch.maximum((X.max(0).values - mean.double()).abs(), (X.min(0).values - mean.double()).abs()) * invstd.double()
    bound = ((w.double().abs() if w is not None else 1.0) * dev + (b.double().abs() if b is not None else 0.0)) / (1.0 - float(np.float32(p)))
    return bound, OB._pow2_scale(float(bound.max()))


def pair64(part):
    """Second stage of the reduce pass: the column sums of the partials [nblk, 2, F] -> (sum_g, sum_gx), and their bound: the double
    additions and the one rounding."""
    s = part.double().sum(0)
    e = U * s.abs() + 2.0 ** -45 * part.double().abs().sum(0)
    return s[0], s[1], e[0], e[1]


def tiles_stats64(part, minmax, pivot, n, eps=1e-5, block_rows=256):
    """colstats_tiles_final_kernel: every block re-based onto the first block's pivot in exact algebra, then mean = P0 + S / n, M2 = Q -
    S^2 / n -> dict(mean, m2, invstd, mn, mx) with bounds (the double arithmetic: 2^-45 of the absolute terms; then one rounding)."""
    nblk = part.shape[0]
    nb = torch.full((nblk, 1), float(block_rows), dtype=F64)
    nb[-1] = n - block_rows * (nblk - 1)
    P0 = pivot[0].double()
    d = pivot.double() - P0
    s_b = part[:, 0].double() + nb * d
    q_b = part[:, 1].double() + 2 * d * part[:, 0].double() + nb * d * d
    S, Q = s_b.sum(0), q_b.sum(0)
    mean = P0 + S / n
    m2 = (Q - S * S / n).clamp(min=0)
    tiny = 2.0 ** -45
    e_S = tiny * (part[:, 0].double().abs() + nb * d.abs()).sum(0)
    e_Q = tiny * (part[:, 1].double().abs() + 2 * (d * part[:, 0].double()).abs() + nb * d * d).sum(0)
    r = {"mean": mean, "m2": m2, "e_mean": U * mean.abs() + e_S / n + tiny * P0.abs()}
    e_m2 = U * m2 + e_Q + (2 * S.abs() * e_S) / n + tiny * (Q.abs() + S * S / n)
    a = m2 / n + float(np.float32(eps))
    rel = (e_m2 / n + 3 * U * a) / a
    r["invstd"] = 1.0 / torch.sqrt(a)
    r["e_invstd"] = r["invstd"] * (0.5 * rel / (1 - rel).clamp(min=0.5) + rel * rel + RSQRT_ERR)
    r["e_m2"] = e_m2
    r["mn"], r["mx"] = minmax[:, 0].min(0).values.double(), minmax[:, 1].max(0).values.double()
    return r


# ------------------------------------------------------------------------------------------------ halves layouts
def fwd_halves_expected(y32, s, F, piece, pieces, mutant=None):
    """The whole [n, pieces * piece] operand as int16 bit patterns: [h1 | h1 | 2^11 h2] (3) or [h1 | 2^11 h2] (2) of float32(y) s, zeros
    in the columns F .. piece - 1 of every piece."""
    h1, h2 = SC.halves_encode(y32.numpy(), s)
    if mutant == 8:
        z = y32.numpy() * np.float32(s)
        h2 = (z - h1.astype(np.float32)).astype(np.float16)
    buf = np.zeros((y32.shape[0], pieces * piece), dtype=np.int16)
    buf[:, :F] = h1.view(np.int16)
    if pieces == 3:
        buf[:, piece:piece + F] = h1.view(np.int16)
    buf[:, (pieces - 1) * piece:(pieces - 1) * piece + F] = h2.view(np.int16)
    return torch.from_numpy(buf)


def fwd_halves_decode(buf16, s, F, piece, pieces):
    f = buf16.contiguous().view(torch.float16).double()
    return (f[:, :F] + f[:, (pieces - 1) * piece:(pieces - 1) * piece + F] / 2048.0) / s


def heads_layout(F, hD, hDP):
    """(ldh, col0, h2_off) of the wider fp16 operand an apply-with-halves case writes into: the block starts col0 = 2 columns (4 bytes,
    not 8) into the row and the second half lies h2_off = H hDP + 2 columns behind the first."""
    H = F // hD
    return 2 + 2 * H * hDP + 2 + 6, 2, H * hDP + 2


def heads_mask(n, F, hD, hDP):
    """True where the operand holds a value (both halves)."""
    ldh, col0, h2 = heads_layout(F, hD, hDP)
    m = torch.zeros(n, ldh, dtype=torch.bool)
    for h in range(F // hD):
        for base in (col0 + h * hDP, col0 + h2 + h * hDP):
            m[:, base:base + hD] = True
    return m


def heads_expected(dx32, s, F, hD, hDP, mutant=None):
    """[n, ldh] int16: SENTINEL16 wherever the contract writes nothing (guards, the gap, the padding columns between hD and hDP)."""
    ldh, col0, h2 = heads_layout(F, hD, hDP)
    step = hD if mutant == 9 else hDP
    h1, h2v = SC.halves_encode(dx32.numpy(), s)
    buf = np.full((dx32.shape[0], ldh), SC.SENTINEL16, dtype=np.int16)
    for h in range(F // hD):
        buf[:, col0 + h * step:col0 + h * step + hD] = h1[:, h * hD:(h + 1) * hD].view(np.int16)
        buf[:, col0 + h2 + h * step:col0 + h2 + h * step + hD] = h2v[:, h * hD:(h + 1) * hD].view(np.int16)
    return torch.from_numpy(buf)


def heads_decode(buf16, s, F, hD, hDP):
    ldh, col0, h2 = heads_layout(F, hD, hDP)
    f = buf16.contiguous().view(torch.float16).double()
    return torch.cat([f[:, col0 + h * hDP:col0 + h * hDP + hD] + f[:, col0 + h2 + h * hDP:col0 + h2 + h * hDP + hD] / 2048.0
                      for h in range(F // hD)], 1) / s


def same_halves(a, b):
    """int16 bit patterns equal, zeros without their sign (a dropped negative entry is -0 or +0 by the order of the gate and the mask's
    product, which the contract leaves open; the second half of an exactly representable value is +0 either way)."""
    zero = torch.tensor(-32768, dtype=torch.int16)
    return torch.equal(torch.where(a == zero, torch.zeros_like(a), a), torch.where(b == zero, torch.zeros_like(b), b))


def halves_bound(ref, e, s):
    return e + 2.0 ** -22 * (ref.abs() + e) + 2.0 ** -36 / s


# ------------------------------------------------------------------------------------------------ checks
def _bits(a, b):
    """float32 a equals float64 b bit for bit (zeros without their sign: relu and a zeroed gradient leave either)."""
    a32, b32 = a.contiguous().float(), b.float()
    return torch.equal(torch.where(a32 == 0, torch.zeros_like(a32), a32).view(torch.int32), torch.where(b32 == 0, torch.zeros_like(b32), b32).view(torch.int32))


def check_values(bad, worst, name, exact, got, want, bound, alt=None):
    """got (float32) against want (float64): bit for bit, or entry for entry under `bound`; alt: a second admissible value per entry."""
    if exact:
        if not _bits(got, want):
            ne = (got.double() != want).nonzero()
            bad.append("%s: %d differ, first %s" % (name, ne.shape[0], [(tuple(t.tolist()), float(got[tuple(t)]), float(want[tuple(t)])) for t in ne[:3]]))
        return
    err = (got.double() - want).abs()
    if alt is not None:
        err = torch.minimum(err, (got.double() - alt).abs())
    if err.numel() == 0:
        return
    if bool(torch.isnan(err).any()) or bool((err > bound).any()):
        at = (torch.isnan(err) | (err > bound)).nonzero()
        bad.append("%s: %d over the bound, first (index, error, bound) %s" % (
            name, at.shape[0], [(tuple(t.tolist()), float(err[tuple(t)]), float(bound[tuple(t)])) for t in at[:3]]))
    if worst is not None:
        worst[name] = max(worst.get(name, 0.0), float((err / bound.clamp(min=1e-300)).max()))


def check_mask(got_y, keep):
    """relu off: y is zero exactly where the mask drops (a kept entry is zero only where pre is: the caller passes inputs without)."""
    return torch.equal(got_y != 0, keep)


# ------------------------------------------------------------------------------------------------ the directed gate test
def gate_emulation(x, mean, invstd, w, b):
    """The two float32 gate expressions of csrc/dense.hip, emulated exactly: forward fmaf(v - mu, invstd w, b) > 0, backward (as the
    three backward sites had it) fmaf((v - mu) invstd, w, b) > 0.  A product of two float32 numbers is exact in float64 and rounding a
    nonzero sum never changes its sign, so the sign of the float64 value IS the sign of the fmaf.  -> (forward gate, backward gate)."""
    x, mean, invstd, w, b = (np.asarray(t, dtype=np.float32) for t in (x, mean, invstd, w, b))
    d = (x - mean).astype(np.float32)
    sw = (invstd * w).astype(np.float32)
    xh = (d * invstd).astype(np.float32)
    fwd = d.astype(np.float64) * sw.astype(np.float64) + b.astype(np.float64) > 0
    bwd = xh.astype(np.float64) * w.astype(np.float64) + b.astype(np.float64) > 0
    return fwd, bwd


@functools.lru_cache(maxsize=None)
def gate_inputs(n_cols=40, steps=64):
    """x [2 steps + 1, n_cols] whose column c holds v = mean + (-b / (invstd w)) stepped by -steps ... +steps float32 ulps, for the n_cols
    of 4 096 seeded (mean, invstd, w, b) on which the two expressions disagree most -> (x, mean, invstd, w, b, share of disagreeing
    entries)."""
    rng = np.random.default_rng(17)
    N = 4096
    invstd = rng.uniform(0.5, 4.0, N).astype(np.float32)
    w = (rng.uniform(0.25, 2.0, N) * rng.choice([-1.0, 1.0], N)).astype(np.float32)
    b = (rng.uniform(0.1, 1.0, N) * rng.choice([-1.0, 1.0], N)).astype(np.float32)
    d0 = (-b / (invstd * w)).astype(np.float32)
    mean = (-d0 * (1 - 2.0 ** -rng.integers(0, 9, N).astype(np.float64)) + rng.choice([0.0, 1.0], N) * rng.normal(0, 1, N)).astype(np.float32)
    v0 = (mean + d0).astype(np.float32)
    sgn = np.where(v0 > 0, 1, -1).astype(np.int32)[None, :]

    def window(centre, half):
        k = np.arange(-half, half + 1, dtype=np.int32)[:, None]
        return (centre.view(np.int32)[None, :] + sgn * k).astype(np.int32).view(np.float32)
    # the quotient's own rounding moves the boundary by many ulps of a small v: find the forward's sign change in a wide window first
    wide = window(v0, 2048)
    f0 = gate_emulation(wide, mean, invstd, w, b)[0]
    change = np.abs(np.diff(f0.astype(np.int8), axis=0))
    ok = (np.abs(v0) > 1e-2) & (change.sum(0) == 1)
    v0 = np.where(ok, wide[np.minimum(change.argmax(0) + 1, 4096), np.arange(N)], v0).astype(np.float32)
    x = window(v0, steps)
    fwd, bwd = gate_emulation(x, mean, invstd, w, b)
    share = np.where(ok, (fwd != bwd).mean(0), 0.0)
    pick = np.sort(np.argsort(-share)[:n_cols])
    x, mean, invstd, w, b = x[:, pick], mean[pick], invstd[pick], w[pick], b[pick]
    fwd, bwd = gate_emulation(x, mean, invstd, w, b)
    assert fwd.any(0).all() and (~fwd).any(0).all(), "every column crosses the boundary"
    return _f(x), _f(mean), _f(invstd), _f(w), _f(b), float((fwd != bwd).mean())
