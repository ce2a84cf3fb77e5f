"""The halves GEMMs (csrc/halves3.hip) and their encoders (csrc/halves.hip) restated in float64, the launch forms their entry points
dispatch to restated in Python, and the case lists of tests/test_halves_host.py and tests/test_halves_gpu.py.

Contracts (include/bot_gnn.h), evaluated from the fp16 BUFFERS a launch is given - never from fp32 originals, so the four pieces of a case
are independent values and a dropped or swapped term is as large as the result:

  NT          C[r, c] = alpha * sum_t sum_i ( a1 b1 + a1 b2 + a2s fp16(2^-11 b1) ),   a2s at a2_off, b2 at b2_off.  The third factor is
              ROUNDED to fp16 (the kernel's v_pk_mul_f16 of the b1 fragment), subnormals included: numpy's float16 rounding here.
              With a second scale alpha = scale_a2[1] scale_b[1] and the partial sum in front of k-step k_split / 32 is multiplied by
              scale_a2[0] scale_a[1].  A fragment-major B is decoded by `frag_index`, written from the header's formula.
  NT grouped  the H3Group formula (a_col0 before k-step k_seg, a_col1 from it on; b_row0, n_valid, c_off), then C * col_scale + col_shift
              (one fused multiply-add), ReLU, max|stored| into the slot set, and per 256-row tile the statistics (pivot = the tile's first
              stored row, sum (v - pivot), sum (v - pivot)^2, min, max) over the rows below m only.  The statistics are held to the
              float64 statistics of the STORED float32 values (`stored_stats`): pivot, min and max bit for bit, the two sums under
              gamma(rows + 2) of their absolute terms - a sum of squares of 2^-11-quantum values is not exact in any regime.
  TN          out[k, p] = scale_x[1] scale_d[1] * sum_rows ( x1 d1 + fp16(2^-11 x1) d2s + x2s fp16(2^-11 d1) ): BOTH second halves are
              stored with their 2^11, and the kernel body applies the 2^-11 to the FIRST half of the other operand in each mixed term (x1s
              = x1 * 2^-11 in front of d2s, d1s = d1 * 2^-11 in front of x2s), each rounded to fp16.  scale_d2 replaces scale_d from column
              p_split on.  Tile lists: x_col0, k_valid, d_col0, p_valid, out_off, ldo, transposed.
  encoders    v = fp32(x s), h1 = fp16(v), h2 = fp16(fp32(fma(x, s, -h1))) (x 2^11 for left operands), order 1's third piece fp16(2^-11 h1).
              For the power-of-two scales halves_scale produces x s is exact and fma(x, s, -h1) = v - h1; only those scales are used.

Two regimes.  EXACT: pieces are small integers (times a power of two), scales powers of two, and `assert_exact` checks, per output entry,
sum |terms| / quantum < 2^24 with quantum the common power of two all terms are multiples of - then every partial sum in any order,
split or not, is a float32 number and the device must return the restatement's bits.  SEEDED: independent normal values; the only error is
float32 accumulation, bounded per entry by gamma(2 nnz + splits + 2) * sum |terms| * alpha, gamma(k) = k u / (1 - k u), u = 2^-23, nnz
the entry's count of non-zero products (a zero product adds nothing).  u is 2^-23 and not 2^-24 because the way the matrix core aligns and
rounds the 32 addends of one v_mfma_f32_16x16x32_f16 is not documented as round-to-nearest; 2 nnz allows each product one alignment and one
accumulation error.

Non-finite data: an infinite or NaN entry poisons exactly the output row (A), column (B), or TN row / column it belongs to.  inf * 0 is
NaN, and a row of B that holds zeros next to the infinite entry of A's row exists in every case here, so what comes out of a poisoned entry
is NaN or +-inf as the float64 restatement says; the tests compare the SET of non-finite entries and, where the restatement is infinite,
its sign."""
import math
import os
from collections import namedtuple

import numpy as np

F16, F32, F64 = np.float16, np.float32, np.float64
U = 2.0 ** -23
SHIFT = 2048.0
BK = 32
TT = 192
GUARD_ROWS = 2                 # rows of NaN in front of and behind every fp16 operand
NAN16 = np.float16("nan")


def gamma(k):
    k = np.asarray(k, dtype=F64)
    return k * U / (1.0 - k * U)


def shifted(h):
    """fp16(2^-11 h) as numpy rounds it (round to nearest even, gradual underflow)."""
    with np.errstate(all="ignore"):
        return (np.asarray(h, dtype=F64) * 2.0 ** -11).astype(F16)


def bits32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=F32)).view(np.int32)


def same_bits(got, ref):
    """Bit equality of two float arrays of one type (-0.0 is not +0.0); two NaNs are equal whatever their payload."""
    got, ref = np.ascontiguousarray(got), np.ascontiguousarray(ref)
    assert got.dtype == ref.dtype and got.shape == ref.shape, (got.dtype, ref.dtype, got.shape, ref.shape)
    iv = np.int32 if got.dtype == F32 else np.int16
    return (got.view(iv) == ref.view(iv)) | (np.isnan(got) & np.isnan(ref))


# ------------------------------------------------------------------------------------------------ dispatch
NT_FORMS = {
    "nt64": "bot::gemm_halves3_nt64_kernel",
    "nt64_frag": "bot::gemm_halves3_nt64_frag_kernel",
    "nt64_bnb": "bot::gemm_halves3_nt64_bnb_kernel",
    "nt64_frag_bnb": "bot::gemm_halves3_nt64_frag_bnb_kernel",
    "nt64_bnreduce": "bot::gemm_halves3_nt64_bnreduce_kernel",
    "nt64_frag_bnreduce": "bot::gemm_halves3_nt64_frag_bnreduce_kernel",
    "nt64_bnapply": "bot::gemm_halves3_nt64_bnapply_kernel",
    "nt64_frag_bnapply": "bot::gemm_halves3_nt64_frag_bnapply_kernel",
    "nt_plain": "bot::gemm_halves3_nt_kernel<256,256,2,4,plain>",
    "nt_ablate": "bot::gemm_halves3_nt_kernel<256,256,2,4,pipelined,ablate>",
    "nt_pipelined": "bot::gemm_halves3_nt_kernel<256,256,2,4,pipelined>",
    "nt64_grouped": "bot::gemm_halves3_nt64_grouped_kernel",
    "nt_grouped": "bot::gemm_halves3_nt_grouped_kernel<256,256,2,4,pipelined>",
}
TN_FORMS = {
    "tn": "bot::gemm_halves3_tn_kernel",
    "tn_grouped128": "bot::gemm_halves3_tn_grouped_kernel<128>",
    "tn_grouped192": "bot::gemm_halves3_tn_grouped_kernel<192>",
}
MODE_128X64, MODE_PLAIN, MODE_ABLATE = 1024, 32, 16      # 16: a mode bit no kernel reads - the ablation build with every switch off


def nt64_wanted():
    return os.environ.get("BOT_NT_KERNEL", "") != "128x64"


def expected_nt(k, mode=0, b_layout=0, bn=None):
    """bot_gemm_halves3_nt{,2,3}_f32 and the deferred pair (bn: None, "store", "reduce", "apply") -> the kernel name, None: refused."""
    force = bool(mode & MODE_128X64)
    mode &= ~MODE_128X64
    frag = "_frag" if b_layout else ""
    if bn is not None:
        if mode or force or k % 64 or not nt64_wanted():
            return None
        return NT_FORMS["nt64" + frag + {"store": "_bnb", "reduce": "_bnreduce", "apply": "_bnapply"}[bn]]
    if b_layout and (mode or k % 64):
        return None
    if mode == 0 and not force and nt64_wanted() and (k // BK) % 2 == 0:
        return NT_FORMS["nt64" + frag]
    if b_layout:
        return None
    if mode & MODE_PLAIN:
        return NT_FORMS["nt_plain"]
    return NT_FORMS["nt_ablate"] if mode else NT_FORMS["nt_pipelined"]


def expected_nt_grouped(groups, k_seg, mode=0, stats=False):
    even = k_seg % 2 == 0 and all(g[4] % 2 == 0 for g in groups)
    nt64 = not (mode & MODE_128X64) and even and nt64_wanted()
    if stats and not nt64:
        return None
    return NT_FORMS["nt64_grouped" if nt64 else "nt_grouped"]


def expected_tn():
    return TN_FORMS["tn"]


def expected_tn_grouped(tiles):
    return TN_FORMS["tn_grouped128" if max(t[3] for t in tiles) <= 128 else "tn_grouped192"]


def expected_kernel(entry, *a, **kw):
    """the kernel name `bot_last_kernel()` reports after a call of `entry` ("nt", "nt_grouped", "tn", "tn_grouped"); None: refused"""
    return {"nt": expected_nt, "nt_grouped": expected_nt_grouped, "tn": expected_tn, "tn_grouped": expected_tn_grouped}[entry](*a, **kw)


def all_forms():
    return set(NT_FORMS.values()) | set(TN_FORMS.values())


def tn_splits(n_rows, kp, pp):
    """csrc/halves3.hip tn_splits and the rounding behind it -> (splits the workspace is sized for, splits launched, rows per split)"""
    tiles = ((kp + TT - 1) // TT) * ((pp + TT - 1) // TT)
    by_rows = n_rows // 4096
    if by_rows < 8:
        s = max(1, by_rows)
    else:
        best_q, best = 1, 0.0
        q = 1
        while q <= 8 and 8 * q <= by_rows:
            wg = q * tiles
            eff = wg / (32.0 * ((wg + 31) // 32))
            if eff > best + 1e-9:
                best, best_q = eff, q
            q += 1
        s = 8 * best_q
    return (s,) + _rps(n_rows, s)


def tn_grouped_splits(n_rows, n_tiles):
    s = max(1, min(8 * max(1, 32 // n_tiles), n_rows // 1024))
    return (s,) + _rps(n_rows, s)


def _rps(n_rows, s):
    rps = ((n_rows + s - 1) // s + 31) // 32 * 32
    return (n_rows + rps - 1) // rps, rps


# bot_amd/gemm.py's routing, restated (its constants are read from the module by the tests that compare)
def piece_of(F, align=64):
    return (F + align - 1) // align * align


def left_order(piece, nodup=True, min_piece=256):
    return 2 if (nodup and piece >= min_piece) else 0


def split_right_order(p, F, right_frag=True, nt_min_cols=192, **kw):
    return 3 if (right_frag and (p >= nt_min_cols or left_order(piece_of(F), **kw) == 2)) else 1


def mm_nt_route(a_order, b_order, p, piece, nt_min_cols=192):
    """-> the kernel name of the hand-written product, or "lib" (the library formulation)"""
    if b_order == 3 or p >= nt_min_cols or a_order == 2:
        return expected_nt(piece, 0, int(b_order == 3))
    return "lib"


def tn_tiles(K, P):
    pt = 128 if (P + 127) // 128 * ((K + 191) // 192) <= 16 else 192
    tiles = [(192 * i, min(192, K - 192 * i), pt * j, min(pt, P - pt * j), 192 * i * P + pt * j, P, 0)
             for i in range((K + 191) // 192) for j in range((P + pt - 1) // pt)]
    return tiles if len(tiles) <= 16 else None


def tn_route(N, K, P, tn_min_out=512 * 1024, narrow=True):
    """the three routes of gemm.tn -> the kernel name, or "lib" """
    KP, PP = piece_of(K), piece_of(P)
    if KP * PP >= tn_min_out:
        return expected_tn()
    if narrow and N >= 8192 and tn_tiles(K, P) is not None:
        return expected_tn_grouped(tn_tiles(K, P))
    return "lib"


# ------------------------------------------------------------------------------------------------ operands
def place16(rows, ld, extra_rows=GUARD_ROWS):
    """An fp16 operand of `rows` rows of pitch ld inside one allocation with guard rows before and behind it; EVERYTHING holds NaN until
    the caller writes the pieces of the contract.  -> (allocation [G + rows + G, ld], view of the operand's rows)"""
    full = np.full((2 * extra_rows + rows, ld), NAN16, dtype=F16)
    return full, full[extra_rows:extra_rows + rows]


def _rng(seed):
    return np.random.default_rng(seed)


def ints(rng, shape, density=1.0, hi=2, unit=1.0):
    """small integers in [-hi, hi] times `unit`, a share 1 - density of them zero"""
    v = rng.integers(-hi, hi + 1, size=shape).astype(F64) * unit
    if density < 1.0:
        v = v * (rng.random(shape) < density)
    return v.astype(F16)


def normals(rng, shape, sigma=48.0, density=1.0):
    v = rng.standard_normal(shape) * sigma
    if density < 1.0:
        v = v * (rng.random(shape) < density)
    return v.astype(F16)


def pow2(e):
    """the (s, 1/s) pair of the scale 2^e as float32"""
    return np.array([2.0 ** e, 2.0 ** -e], dtype=F32)


# ------------------------------------------------------------------------------------------------ the three-term sums
Sum3 = namedtuple("Sum3", "val ab nz")      # float64 value, sum of |terms|, count of non-zero products (ab / nz: None when not wanted)


def _mm(a, b, left_t):
    return a.T @ b if left_t else a @ b.T


def three(l1, l2s, r1, r2, tn, mutant=None, want_bound=True):
    """NT (tn False): rows of l times rows of r,  l1 r1 + l1 r2 + l2s fp16(2^-11 r1).
    TN (tn True): columns of l times columns of r over the common rows,  l1 r1 + fp16(2^-11 l1) r2s + l2s fp16(2^-11 r1)."""
    L1, L2, R1, R2 = (np.asarray(t, dtype=F64) for t in (l1, l2s, r1, r2))
    R1S = shifted(r2 if mutant == "third_b2" else r1).astype(F64)
    LM = shifted(l1).astype(F64) if tn else L1
    terms = [(L1, R1), (LM, R2), (L2, R1S)]
    if mutant == "drop_a1b2":
        terms.pop(1)
    elif mutant == "drop_a2b1":
        terms.pop(2)
    with np.errstate(all="ignore"):
        val = sum(_mm(a, b, tn) for a, b in terms) + 0.0     # an accumulator starts at +0: a sum of zero products is +0, whatever their signs
        if not want_bound:
            return Sum3(val, None, None)
        ab = sum(_mm(np.abs(a), np.abs(b), tn) for a, b in terms)
        nz = sum(_mm((a != 0).astype(F64), (b != 0).astype(F64), tn) for a, b in terms)
    return Sum3(val, ab, nz)


def _add(s, t, f=1.0):
    if t is None:
        return Sum3(s.val * f, None if s.ab is None else s.ab * abs(f), s.nz)
    with np.errstate(all="ignore"):
        return Sum3(s.val * f + t.val, None if s.ab is None else s.ab * abs(f) + t.ab, None if s.nz is None else s.nz + t.nz)


# ------------------------------------------------------------------------------------------------ NT, plain
NT = namedtuple("NT", "m n K dup b2x frag k_split r_exp pad off regime third bn sa sb tag seed")
NT.__new__.__defaults__ = (False, 0, False, 0, 7, 0, 0, "exact", False, False, 3, -2, "", 0)


def frag_index(n, piece):
    """include/bot_gnn.h "FRAGMENT-MAJOR layout": element (row r, column c) of h1 at halves ((t T + s) 64 + l) 8 + (c & 7) with t = r >> 4,
    s = c >> 5, l = (r & 15) + 16 ((c & 31) >> 3), T = piece / 32; h2 ceil(n / 16) T 512 halves behind.  -> (index [rows16, piece], region)"""
    rows16 = (n + 15) // 16 * 16
    r = np.arange(rows16)[:, None]
    c = np.arange(piece)[None, :]
    T = piece // 32
    idx = (((r >> 4) * T + (c >> 5)) * 64 + ((r & 15) + 16 * ((c & 31) >> 3))) * 8 + (c & 7)
    return idx, (rows16 // 16) * T * 512


def frag_pack(b1, b2, outside):
    """[n, piece] halves -> the fragment-major buffer (flat); the rows of the last 16-row tile beyond n hold `outside`"""
    n, piece = b1.shape
    idx, region = frag_index(n, piece)
    flat = np.full(2 * region, outside, dtype=F16)
    flat[idx[:n]] = b1
    flat[region + idx[:n]] = b2
    return flat


def frag_unpack(flat, n, piece):
    idx, region = frag_index(n, piece)
    return flat[idx[:n]], flat[region + idx[:n]]


class NTOps:
    """The operands of an NT case: A [m, lda] (a1 at column 0, a2s at a2_off), B [n, ldb] (b1, b2 at b2_off) or its fragment-major buffer,
    the scale pairs; everything else in the allocations holds `outside` (NaN, or 0 for the never-read comparison)."""


def make_nt(c, outside=NAN16):
    rng = _rng(1000 + c.seed)
    o = NTOps()
    o.c = c
    K = c.K
    piece = K
    o.a2_off = 2 * piece if c.dup else piece
    o.lda = o.a2_off + piece + (8 if c.dup else 0)
    o.b2_off = K + c.b2x
    o.ldb = o.b2_off + K + (8 if c.b2x else 0)
    if c.regime == "exact":
        dens = 1.0 if not c.k_split else 0.2
        hi = 2 if not c.k_split else 1
        a1, a2 = ints(rng, (c.m, K), dens, hi), ints(rng, (c.m, K), dens, hi)
        b1, b2 = ints(rng, (c.n, K), dens, hi), ints(rng, (c.n, K), dens, hi)
    elif c.regime == "subnormal":
        # only the third term lives: a2s small integers, b1 = (2^10 + j) 2^-14 in [2^-4, 2^-3) - its 2^-11 multiple is an fp16 subnormal
        # that needs ROUNDING for odd j (quantum 2^-24)
        a1, b2 = np.zeros((c.m, K), F16), np.zeros((c.n, K), F16)
        a2 = ints(rng, (c.m, K), 0.5, 2)
        b1 = ((1024 + rng.integers(0, 1024, size=(c.n, K))) * 2.0 ** -14 * rng.choice([-1.0, 1.0], size=(c.n, K))).astype(F16)
    else:
        a1, a2, b1, b2 = (normals(rng, s) for s in ((c.m, K), (c.m, K), (c.n, K), (c.n, K)))
        if c.third:
            sc = np.where(np.arange(c.n) % 3 == 0, 1e-3, 1.0)[:, None]
            b1, b2 = (b1.astype(F64) * sc).astype(F16), (b2.astype(F64) * sc).astype(F16)
    o.afull, o.A = place16(c.m, o.lda)
    o.afull[...] = outside
    o.A[:, :K], o.A[:, o.a2_off:o.a2_off + K] = a1, a2
    if c.frag:
        o.bfull = o.B = frag_pack(b1, b2, outside)
    else:
        o.bfull, o.B = place16(c.n, o.ldb)
        o.bfull[...] = outside
        o.B[:, :K], o.B[:, o.b2_off:o.b2_off + K] = b1, b2
    o.sa, o.sb = pow2(c.sa), pow2(c.sb)
    o.sa2 = pow2(c.sa + c.r_exp) if c.k_split else None
    return o


def nt_pieces(o):
    c = o.c
    a1, a2 = o.A[:, :c.K], o.A[:, o.a2_off:o.a2_off + c.K]
    if c.frag:
        b1, b2 = frag_unpack(o.B, c.n, c.K)
    else:
        b1, b2 = o.B[:, :c.K], o.B[:, o.b2_off:o.b2_off + c.K]
    return a1, a2, b1, b2


NT_MUTANTS = ("drop_a1b2", "drop_a2b1", "third_b2", "skip_last_kstep", "rescale_late", "alpha_from_scale_a")


def nt_reference(o, mutant=None, want_bound=True):
    """-> Sum3 of the [m, n] result, alpha applied (ab: sum |terms| * alpha)"""
    c = o.c
    a1, a2, b1, b2 = nt_pieces(o)
    K = c.K - BK if mutant == "skip_last_kstep" else c.K
    m3 = mutant if mutant in ("drop_a1b2", "drop_a2b1", "third_b2") else None

    def part(lo, hi):
        return three(a1[:, lo:hi], a2[:, lo:hi], b1[:, lo:hi], b2[:, lo:hi], False, m3, want_bound)
    if not c.k_split:
        s, alpha = part(0, K), F32(o.sa[1]) * F32(o.sb[1])
    else:
        k2 = min(c.k_split + (BK if mutant == "rescale_late" else 0), K)
        r = float(F32(o.sa2[0]) * F32(o.sa[1]))
        s = _add(part(0, k2), part(k2, K) if k2 < K else None, r)
        if k2 >= K:                                 # (a rescale that never happens: the late mutant at the last k-step)
            s = part(0, K)
        alpha = F32((o.sa if mutant == "alpha_from_scale_a" else o.sa2)[1]) * F32(o.sb[1])
    return _add(s, None, float(alpha))


def exact_premise(s, quantum):
    """Every entry's sum of |terms| is below 2^24 quanta: any partial sum in any order is a float32 number."""
    assert np.all(np.isfinite(s.ab)) and float((s.ab / quantum).max()) < 2.0 ** 24, float((s.ab / quantum).max())
    assert np.array_equal(s.val, np.round(s.val / quantum) * quantum), "a term is no multiple of the quantum"
    assert np.array_equal(s.val.astype(F32).astype(F64), s.val)


def nt_quantum(o):
    c = o.c
    alpha = float((o.sa2 if c.k_split else o.sa)[1]) * float(o.sb[1])
    r = 2.0 ** min(0, c.r_exp) if c.k_split else 1.0
    return (2.0 ** -24 if c.regime == "subnormal" else 2.0 ** -11) * r * alpha


def seeded_bound(s, splits):
    return gamma(2.0 * s.nz + splits + 2.0) * s.ab


def nt_store_path(c):
    pitch = c.n + c.pad
    if pitch % 4 == 0 and c.off % 4 == 0:
        return "float4"
    return "float2" if (pitch % 2 == 0 and c.off % 2 == 0) else "scalar"


def nt_modes(c):
    """the launches of one plain case: the dispatched form, and for a row-major B the forced 128x64 form, the plain loop and the ablation build"""
    return (0,) if c.frag else (0, MODE_128X64, MODE_PLAIN, MODE_ABLATE)


def nt_cases():
    L = []
    i = [0]

    def add(**kw):
        i[0] += 1
        L.append(NT(seed=i[0], **kw))
    for m in (1, 15, 255, 256, 257, 513, 2049):                                  # row tile edges; 2049: the ninth row tile (second XCD group)
        add(m=m, n=33, K=64, tag="m")
    for n in (1, 15, 16, 17, 31, 32, 33, 255, 256, 257, 513):                     # fragment / wave / tile edges of the columns
        add(m=17, n=n, K=128, dup=n % 2 == 0, tag="n")
    for K in (32, 64, 96, 128, 192, 256):                                          # 1 / 3 k-steps: 128x64; 64: the tail only; 128 / 192: 2 / 3 iterations
        add(m=257, n=33, K=K, dup=K == 96, tag="K")
        add(m=33, n=257, K=K, regime="seeded", third=K % 64 == 0, tag="K")
    add(m=40, n=50, K=64, b2x=72, tag="b2_off>K")
    add(m=40, n=50, K=128, b2x=8, dup=True, regime="seeded", tag="b2_off>K")
    for n in (15, 33, 250):                                                        # fragment-major B, n no multiple of 16
        add(m=258, n=n, K=128, frag=True, tag="frag")
        add(m=31, n=n, K=192, frag=True, regime="seeded", third=True, tag="frag")
    for K in (128, 192):                                                           # the second scale at EVERY k-step
        for j, ks in enumerate(range(32, K, 32)):
            add(m=257, n=40, K=K, k_split=ks, r_exp=7 if j % 2 else -7, dup=j % 2 == 0, tag="k_split")
            add(m=40, n=257, K=K, k_split=ks, r_exp=-7 if j % 2 else 7, frag=True, regime="seeded", tag="k_split")
    add(m=100, n=40, K=96, k_split=64, r_exp=7, tag="k_split")                     # the 128x64 form's own rescale site, odd k-step count
    for (n, pad, off) in ((257, 3, 0), (257, 1, 2), (257, 0, 0), (257, 3, 1), (256, 0, 0), (254, 0, 2), (254, 2, 0), (256, 0, 3)):
        add(m=33, n=n, K=64, pad=pad, off=off, tag="store")
    for (n, K, frag) in ((250, 64, False), (250, 128, True), (34, 192, False), (258, 256, True)):   # the BatchNorm-backward forms (n even)
        add(m=257, n=n, K=K, frag=frag, bn=True, dup=False, tag="bn")
    add(m=300, n=36, K=128, frag=False, bn=True, k_split=64, r_exp=7, tag="bn")
    add(m=64, n=48, K=64, sa=60, sb=60, tag="scale clamp")                         # alpha = 2^-120
    add(m=64, n=48, K=64, sa=-86, sb=60, tag="scale clamp")                        # alpha = 2^26
    add(m=64, n=48, K=64, regime="subnormal", tag="subnormal")
    add(m=64, n=48, K=128, regime="subnormal", frag=True, tag="subnormal")
    return L


def nt_paths(c):
    p = {"store:" + nt_store_path(c), "left:dup" if c.dup else "left:nodup", "regime:" + c.regime}
    steps = c.K // BK
    p.add("nt64:%diter" % (steps // 2) if steps % 2 == 0 else "128x64:%dsteps" % steps)
    if c.m > 2048:
        p.add("row tile 9")
    if c.b2x:
        p.add("b2_off>K")
    if c.frag:
        p.add("frag" if c.n % 16 == 0 else "frag:ragged")
    if c.k_split:
        ks = c.k_split // BK
        p |= {"k_split:odd" if ks % 2 else "k_split:even", "k_split:r%+d" % c.r_exp}
        if ks == 1:
            p.add("k_split:first")
        if ks == steps - 1:
            p.add("k_split:last")
    if c.bn:
        p.add("bn")
    for x in (c.m, c.n):
        if x % 256 == 1 and x > 1:
            p.add("tile+1")
    return p


NT_PATHS = {"store:float4", "store:float2", "store:scalar", "left:dup", "left:nodup", "regime:exact", "regime:seeded", "regime:subnormal", "nt64:1iter",
            "nt64:2iter", "nt64:3iter", "nt64:4iter", "128x64:1steps", "128x64:3steps", "row tile 9", "b2_off>K", "frag:ragged", "k_split:odd",
            "k_split:even", "k_split:first", "k_split:last", "k_split:r+7", "k_split:r-7", "bn", "tile+1"}


# ------------------------------------------------------------------------------------------------ NT, grouped
NG = namedtuple("NG", "m groups k_seg lda a2_off b_rows ldb b2_off width pad off cs ch relu absmax stats mode regime tag seed")


def make_ng(c, outside=NAN16):
    rng = _rng(2000 + c.seed)
    o = NTOps()
    o.c = c
    o.afull, o.A = place16(c.m, c.lda)
    o.bfull, o.B = place16(c.b_rows, c.ldb)
    o.afull[...] = outside
    o.bfull[...] = outside
    # the contract's index set: A columns of every group's two ranges (both halves), B rows / columns of every group
    acols = np.zeros(c.lda, bool)
    bmask = np.zeros((c.b_rows, c.ldb), bool)
    for (b_row0, n_valid, a_col0, a_col1, k_steps, c_off) in c.groups:
        for t in range(k_steps):
            col = (a_col0 if t < c.k_seg else a_col1) + BK * t
            acols[col:col + BK] = acols[c.a2_off + col:c.a2_off + col + BK] = True
        bmask[b_row0:b_row0 + n_valid, :BK * k_steps] = True
        bmask[b_row0:b_row0 + n_valid, c.b2_off:c.b2_off + BK * k_steps] = True
    gen = (lambda s: ints(rng, s, 0.6)) if c.regime == "exact" else (lambda s: normals(rng, s))
    o.A[:, acols] = gen((c.m, int(acols.sum())))
    o.B[bmask] = gen((int(bmask.sum()),))
    o.acols, o.bmask = acols, bmask
    o.sa, o.sb = pow2(2), pow2(-1)
    W = c.width
    if c.regime == "exact":
        o.cs = rng.choice([-2.0, -1.0, 0.5, 1.0, 2.0], size=W).astype(F32) if c.cs else None
        o.ch = rng.integers(-3, 4, size=W).astype(F32) if c.ch else None
    else:
        o.cs = (rng.standard_normal(W) + 0.5).astype(F32) if c.cs else None
        o.ch = (rng.standard_normal(W) * 500).astype(F32) if c.ch else None
    return o


NG_MUTANTS = ("a_col0_after_k_seg", "c_off_plus_one", "stats_with_clamped_rows")


def ng_reference(o, mutant=None, want_bound=True):
    """-> dict: val / bound [m, width] float64 (NaN where nothing is written), written [m, width] bool, absmax, and per 256-row tile the
    statistics of `val` (pivot, sum, sumsq, min, max: [tiles, width], NaN at unwritten columns)"""
    c = o.c
    m, W = c.m, c.width
    val = np.full((m, W), np.nan)
    ab = np.full((m, W), np.nan)
    nz = np.full((m, W), np.nan)
    written = np.zeros((m, W), bool)
    alpha = float(F32(o.sa[1]) * F32(o.sb[1]))
    for (b_row0, n_valid, a_col0, a_col1, k_steps, c_off) in c.groups:
        s = None
        for t in range(k_steps):
            col = (a_col0 if (t < c.k_seg or mutant == "a_col0_after_k_seg") else a_col1) + BK * t
            rows = slice(b_row0, b_row0 + n_valid)
            p = three(o.A[:, col:col + BK], o.A[:, c.a2_off + col:c.a2_off + col + BK], o.B[rows, BK * t:BK * t + BK],
                      o.B[rows, c.b2_off + BK * t:c.b2_off + BK * t + BK], False, None, want_bound)
            s = p if s is None else _add(s, p)
        s = _add(s, None, alpha)
        co = c_off + (1 if mutant == "c_off_plus_one" else 0)
        cols, nv = slice(co, min(co + n_valid, W)), min(co + n_valid, W) - co        # (clipped: the shifted mutant at the last column)
        val[:, cols], written[:, cols] = s.val[:, :nv], True
        if want_bound:
            ab[:, cols], nz[:, cols] = s.ab[:, :nv], s.nz[:, :nv]
    r = {"written": written, "prod": val.copy(), "ab": ab, "nz": nz}
    with np.errstate(all="ignore"):
        if o.cs is not None or o.ch is not None or c.relu:
            cs = np.ones(W) if o.cs is None else o.cs.astype(F64)
            ch = np.zeros(W) if o.ch is None else o.ch.astype(F64)
            val = val * cs + ch
            if c.relu:
                val = np.where(val > 0, val, 0.0)                    # fmaxf(v, 0): NaN -> 0
            if want_bound:          # the product's error through the multiply-add (one more rounding), ReLU is 1-Lipschitz
                e = seeded_bound(Sum3(None, ab, nz), 1) * np.abs(cs)
                r["bound"] = e + U * (np.abs(r["prod"] * cs) + e + np.abs(ch))
        elif want_bound:
            r["bound"] = seeded_bound(Sum3(None, ab, nz), 1)
    r["val"] = val
    fin = np.where(written & ~np.isnan(val), np.abs(val), 0.0)
    r["absmax"] = float(fin.max()) if fin.size else 0.0
    r.update(tile_stats(val, written, m, clamped=mutant == "stats_with_clamped_rows"))
    return r


def tile_stats(val, written, m, clamped=False):
    """per 256-row tile and written column: pivot = the first row's value, sum (v - pivot), sum (v - pivot)^2, min, max over the tile's rows
    below m (clamped: the mutant that lets the last row stand in for the rows of the tile beyond m, as a kernel that forgot `row < M` would)"""
    tiles, W = (m + 255) // 256, val.shape[1]
    out = {k: np.full((tiles, W), np.nan) for k in ("pivot", "sum", "sumsq", "min", "max")}
    for t in range(tiles):
        v = val[256 * t:min(256 * (t + 1), m)]
        if clamped and v.shape[0] < 256:
            v = np.concatenate([v, np.repeat(v[-1:], 256 - v.shape[0], 0)])
        d = v - v[0]
        out["pivot"][t], out["sum"][t], out["sumsq"][t], out["min"][t], out["max"][t] = v[0], d.sum(0), (d * d).sum(0), v.min(0), v.max(0)
    col = written[0]
    for k in out:
        out[k][:, ~col] = np.nan
    return out


def stored_stats(C, written, m):
    """tile_stats of the float32 values a launch stored (C [m, width]) with the bounds of their float32 evaluation: d = fl(v - pivot) is one
    rounding, each sum adds one per row (the squares ride in a fused multiply-add)"""
    r = tile_stats(C.astype(F64), written, m)
    tiles = (m + 255) // 256
    for k in ("e_sum", "e_sumsq", "a_sum", "a_sumsq"):
        r[k] = np.zeros_like(r["sum"])
    for t in range(tiles):
        v = C[256 * t:min(256 * (t + 1), m)].astype(F64)
        d = np.abs(v - v[0])
        g = gamma(v.shape[0] + 2)
        r["a_sum"][t], r["a_sumsq"][t] = d.sum(0), (d * d).sum(0)          # the sums of the absolute terms
        r["e_sum"][t], r["e_sumsq"][t] = g * r["a_sum"][t], g * r["a_sumsq"][t]
    return r


def ng_cases():
    L = []

    def add(m, groups, k_seg, b_rows, width, kmax, i, pad=0, off=0, cs=False, ch=False, relu=False, absmax=False, stats=False, mode=0, regime="exact",
            tag="", a_extra=0):
        a_hi = max(max(g[2], g[3]) + BK * g[4] for g in groups) + a_extra
        a2_off = (a_hi + 7) // 8 * 8
        L.append(NG(m, tuple(groups), k_seg, 2 * a2_off + 8, a2_off, b_rows, 2 * BK * kmax + 16, BK * kmax + 8, width, pad, off, cs, ch, relu, absmax, stats,
                    mode, regime, tag, i))
    # one group, every n_valid, the three k_seg of the 256x32 form (0, 2, k_steps)
    for i, (nv, k_seg) in enumerate(((1, 0), (31, 2), (250, 4), (256, 2))):
        add(257, [(3, nv, 0, 40, 4, 0)], k_seg, 3 + nv + 2, nv, 4, i, absmax=True, stats=True, regime="exact" if i % 2 == 0 else "seeded", tag="1 group")
    # two groups with different k_steps, overlapping A ranges, output bases 4-, 8- and 16-byte aligned (off + c_off), all epilogue combinations
    combos = [(cs, ch, relu) for cs in (False, True) for ch in (False, True) for relu in (False, True)]
    for i, (cs, ch, relu) in enumerate(combos):
        off, c1 = ((0, 32), (2, 34), (1, 31), (0, 33))[i % 4]
        add(270 - 200 * (i % 2), [(0, 31, 0, 64, 2, 0), (40, 250, 32, 8, 4, c1)], 2, 300, c1 + 250, 4, 10 + i, pad=i % 3, off=off, cs=cs, ch=ch, relu=relu,
            absmax=True, stats=i % 2 == 0, regime="exact" if i < 6 else "seeded", tag="2 groups")
    # twelve groups
    g12 = [(20 * j, 16 + (j % 3), 8 * j, 64 + 8 * j, 2 + 2 * (j % 2), 20 * j) for j in range(12)]
    add(513, g12, 2, 260, 240, 4, 30, absmax=True, stats=True, cs=True, tag="12 groups")
    add(300, g12, 2, 260, 240, 4, 31, regime="seeded", ch=True, relu=True, absmax=True, tag="12 groups")
    # the 128x64 form: an odd k_seg, an odd k_steps, and the forced form on an even list
    add(257, [(0, 31, 0, 72, 3, 0), (31, 250, 8, 16, 4, 32)], 1, 290, 282, 4, 40, absmax=True, cs=True, relu=True, tag="128x64 odd k_seg")
    add(100, [(0, 256, 0, 0, 3, 0)], 0, 256, 256, 3, 41, regime="seeded", tag="128x64 odd k_steps")
    add(257, [(3, 250, 0, 40, 4, 0)], 2, 260, 250, 4, 42, mode=MODE_128X64, absmax=True, ch=True, tag="128x64 forced")
    return L


def ng_paths(c):
    p = {"groups:%d" % len(c.groups), "k_seg:%s" % ("0" if c.k_seg == 0 else "all" if all(c.k_seg >= g[4] for g in c.groups) else "odd" if c.k_seg % 2 else "mid"),
         "epi:%d%d%d" % (c.cs, c.ch, c.relu), "regime:" + c.regime}
    for g in c.groups:
        p.add("n_valid:%d" % g[1]) if g[1] in (1, 31, 250, 256) else None
        base = (c.off + g[5]) % 4
        p.add("base:%d" % (16 if base == 0 else 8 if base == 2 else 4))
    if len({g[4] for g in c.groups}) > 1:
        p.add("k_steps differ")
    if c.stats and c.m % 256:
        p.add("stats ragged")
    if c.absmax:
        p.add("absmax")
    return p


NG_PATHS = ({"groups:1", "groups:2", "groups:12", "k_seg:0", "k_seg:mid", "k_seg:all", "k_seg:odd", "n_valid:1", "n_valid:31", "n_valid:250", "n_valid:256",
             "base:4", "base:8", "base:16", "k_steps differ", "stats ragged", "absmax", "regime:exact", "regime:seeded"} |
            {"epi:%d%d%d" % (a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1)})


# ------------------------------------------------------------------------------------------------ TN
TN = namedtuple("TN", "n K P xdup ddup ldo_pad p_split r_exp density regime third tag seed")
TN.__new__.__defaults__ = (False, False, 0, 0, 5, 1.0, "exact", False, "", 0)


def make_tn(c, outside=NAN16):
    rng = _rng(3000 + c.seed)
    o = NTOps()
    o.c = c
    o.kp, o.pp = piece_of(c.K), piece_of(c.P)
    o.x2_off, o.d2_off = (2 if c.xdup else 1) * o.kp, (2 if c.ddup else 1) * o.pp
    o.ldx, o.ldd = o.x2_off + o.kp, o.d2_off + o.pp
    o.xfull, o.X = place16(c.n, o.ldx)
    o.dfull, o.D = place16(c.n, o.ldd)
    o.xfull[...] = outside
    o.dfull[...] = outside
    gen = (lambda s: ints(rng, s, c.density)) if c.regime == "exact" else (lambda s: normals(rng, s, density=c.density))
    for (V, off, w, wp) in ((o.X, 0, c.K, o.kp), (o.X, o.x2_off, c.K, o.kp), (o.D, 0, c.P, o.pp), (o.D, o.d2_off, c.P, o.pp)):
        V[:, off:off + wp] = 0                       # the zero padding of a piece is part of the contract (the tiles read it)
        V[:, off:off + w] = gen((c.n, w))
    if c.third:
        sc = np.where(np.arange(c.P) % 3 == 0, 1e-3, 1.0)[None, :]
        for off in (0, o.d2_off):
            o.D[:, off:off + c.P] = (o.D[:, off:off + c.P].astype(F64) * sc).astype(F16)
    o.sx, o.sd = pow2(1), pow2(-3)
    o.sd2 = pow2(-3 + c.r_exp) if c.p_split else None
    return o


TN_MUTANTS = ("p_split_one_quad_late", "drop_a1b2", "drop_a2b1")


def tn_alpha(o, mutant=None):
    c = o.c
    alpha = np.full(c.P, float(F32(o.sx[1]) * F32(o.sd[1])))
    if c.p_split:
        alpha[c.p_split + (4 if mutant == "p_split_one_quad_late" else 0):] = float(F32(o.sx[1]) * F32(o.sd2[1]))
    return alpha


def tn_reference(o, mutant=None, want_bound=True):
    c = o.c
    m3 = mutant if mutant in ("drop_a1b2", "drop_a2b1") else None
    s = three(o.X[:, :c.K], o.X[:, o.x2_off:o.x2_off + c.K], o.D[:, :c.P], o.D[:, o.d2_off:o.d2_off + c.P], True, m3, want_bound)
    alpha = tn_alpha(o, mutant)
    with np.errstate(all="ignore"):
        return Sum3(s.val * alpha, None if s.ab is None else s.ab * alpha, s.nz)


def tn_cases():
    L = []
    i = [0]

    def add(**kw):
        i[0] += 1
        L.append(TN(seed=i[0], **kw))
    for n in (1, 31, 32, 33, 4095):                                                # one split: 1, 1, 1, 2, 128 steps
        add(n=n, K=65, P=63, xdup=n % 2 == 0, density=0.3 if n > 1000 else 1.0, tag="rows")
    add(n=8192, K=40, P=64, density=0.05, tag="rows")                              # 2 splits
    add(n=8193, K=64, P=40, density=0.05, ddup=True, regime="seeded", tag="rows")  # 2 splits, a ragged second one
    add(n=32773, K=64, P=64, density=0.02, tag="rows")                             # 8 splits
    add(n=262149, K=64, P=64, density=0.03, tag="rows")                            # 64 splits, 64-wide pieces without the duplicate
    add(n=262149, K=64, P=64, density=0.03, regime="seeded", third=True, tag="rows")
    widths = (1, 63, 64, 65, 191, 192, 193, 250, 385)
    for j, w in enumerate(widths):                                                 # every width on both axes, paired with a rotated partner
        v = widths[(j + 4) % len(widths)]
        add(n=70, K=w, P=v, xdup=j % 2 == 0, ddup=j % 3 == 0, ldo_pad=j % 4, regime="exact" if j % 2 == 0 else "seeded", third=j % 4 == 1, tag="widths")
        add(n=33, K=v, P=w, xdup=j % 3 == 1, ddup=j % 2 == 1, regime="seeded" if j % 2 == 0 else "exact", tag="widths")
    for (P, ps) in ((250, 4), (250, 192), (255, 252), (385, 192), (447, 444)):      # the second scale: at 4, at a tile boundary, at pp - 4
        add(n=40, K=65, P=P, p_split=ps, r_exp=5 if ps % 8 else -5, ldo_pad=3, tag="p_split")
        add(n=40, K=65, P=P, p_split=ps, regime="seeded", tag="p_split")
    return L


def tn_paths(c):
    s = tn_splits(c.n, piece_of(c.K), piece_of(c.P))[1]
    p = {"splits:%d" % s, "x:dup" if c.xdup else "x:nodup", "d:dup" if c.ddup else "d:nodup", "regime:" + c.regime, "K:%d" % c.K, "P:%d" % c.P}
    if c.ldo_pad:
        p.add("ldo>P")
    if c.p_split:
        pp = piece_of(c.P)
        p.add("p_split:" + ("4" if c.p_split == 4 else "tile" if c.p_split % TT == 0 else "pp-4" if c.p_split == pp - 4 else "other"))
    return p


TN_PATHS = ({"splits:1", "splits:2", "splits:8", "splits:64", "x:dup", "x:nodup", "d:dup", "d:nodup", "regime:exact", "regime:seeded", "ldo>P", "p_split:4",
             "p_split:tile", "p_split:pp-4"} | {"K:%d" % w for w in (1, 63, 64, 65, 191, 192, 193, 250, 385)} |
            {"P:%d" % w for w in (1, 63, 64, 65, 191, 192, 193, 250, 385)})


# ------------------------------------------------------------------------------------------------ TN, grouped
TG = namedtuple("TG", "n tiles ldx x2_off ldd d2_off out_floats density regime tag seed")


def make_tg(c, outside=NAN16):
    rng = _rng(4000 + c.seed)
    o = NTOps()
    o.c = c
    o.xfull, o.X = place16(c.n, c.ldx)
    o.dfull, o.D = place16(c.n, c.ldd)
    o.xfull[...] = outside
    o.dfull[...] = outside
    xc, dc = np.zeros(c.ldx, bool), np.zeros(c.ldd, bool)
    for (x0, kv, d0, pv, out_off, ldo, tr) in c.tiles:
        xc[x0:x0 + kv] = xc[c.x2_off + x0:c.x2_off + x0 + kv] = True
        dc[d0:d0 + pv] = dc[c.d2_off + d0:c.d2_off + d0 + pv] = True
    gen = (lambda s: ints(rng, s, c.density)) if c.regime == "exact" else (lambda s: normals(rng, s, density=c.density))
    o.X[:, xc], o.D[:, dc] = gen((c.n, int(xc.sum()))), gen((c.n, int(dc.sum())))
    o.sx, o.sd = pow2(2), pow2(-4)
    return o


TG_MUTANTS = ("ignore_transposed",)


def tg_reference(o, mutant=None, want_bound=True):
    """-> (val, bound-or-None, written) over the flat output buffer"""
    c = o.c
    val, ab, nz = (np.full(c.out_floats, np.nan) for _ in range(3))
    written = np.zeros(c.out_floats, bool)
    alpha = float(F32(o.sx[1]) * F32(o.sd[1]))
    for (x0, kv, d0, pv, out_off, ldo, tr) in c.tiles:
        s = three(o.X[:, x0:x0 + kv], o.X[:, c.x2_off + x0:c.x2_off + x0 + kv], o.D[:, d0:d0 + pv], o.D[:, c.d2_off + d0:c.d2_off + d0 + pv], True, None,
                  want_bound)
        k, p = np.arange(kv)[:, None], np.arange(pv)[None, :]
        idx = out_off + (p * ldo + k if (tr and mutant != "ignore_transposed") else k * ldo + p)
        ok = idx < c.out_floats                     # (all of them, except under the mutant)
        val[idx[ok]], written[idx[ok]] = (s.val * alpha)[ok], True
        if want_bound:
            ab[idx[ok]], nz[idx[ok]] = (s.ab * alpha)[ok], s.nz[ok]
    return val, (Sum3(None, ab, nz) if want_bound else None), written


def tg_cases():
    L = []

    def add(n, tiles, i, density=1.0, regime="exact", tag="", dup=False):
        # pieces just wide enough for the tiles' valid columns: a 192-column read window then runs into the next piece, the next row and,
        # in the last row, past the operand's end (the buffer descriptor returns zeros there)
        xw, dw = (max(t[0] + t[1] for t in tiles) + 7) // 8 * 8, (max(t[2] + t[3] for t in tiles) + 7) // 8 * 8
        x2, d2 = (2 * xw if dup else xw), dw
        size = max(t[4] + ((t[3] - 1) * t[5] + t[1] if t[6] else (t[1] - 1) * t[5] + t[3]) for t in tiles) + 5
        L.append(TG(n, tuple(tiles), x2 + xw, x2, d2 + dw, d2, size, density, regime, tag, i))
    # PT 128, one tile, every valid width; the 192-column read window runs past k_valid into the second half's piece
    for i, (kv, pv) in enumerate(((1, 128), (127, 1), (128, 127), (129, 128), (191, 127), (192, 128))):
        add(1023 + (i % 2), [(0, kv, 0, pv, 3 * (i % 2), (kv if i % 2 else pv) + (i % 3), i % 2)], i, regime="exact" if i % 2 == 0 else "seeded", tag="PT128", density=0.3)
    # PT 192 (a p_valid above 128)
    for i, (kv, pv) in enumerate(((192, 192), (129, 191), (1, 129), (191, 192))):
        add(70 + 1000 * (i % 2), [(8, kv, 16, pv, 0, (kv if i % 2 else pv) + 1, i % 2)], 10 + i, regime="exact" if i % 2 else "seeded", tag="PT192",
            density=0.3, dup=i == 0)
    # sixteen tiles, transposed and plain in one list, at 2049 rows (2 splits) and 40000 rows (16 splits)
    t16, off = [], 0
    for j in range(16):
        kv, pv = (1, 127, 128, 129, 191, 192)[j % 6], (128, 1, 127, 96, 64, 33)[j % 6]
        ldo = (kv if j % 2 else pv) + (j % 3)
        t16.append((8 * j, kv, 8 * (15 - j), pv, off, ldo, j % 2))
        off += (pv if j % 2 else kv) * ldo
    add(2049, t16, 20, density=0.1, tag="16 tiles")
    add(40000, t16, 21, density=0.02, regime="seeded", tag="16 tiles")
    add(40000, t16[:3], 22, density=0.005, tag="3 tiles: 39 splits sized, 38 launched")
    return L


def tg_paths(c):
    p = {"PT:%d" % (128 if max(t[3] for t in c.tiles) <= 128 else 192), "tiles:%d" % len(c.tiles), "regime:" + c.regime,
         "splits:%d" % tn_grouped_splits(c.n, len(c.tiles))[1]}
    if len({t[6] for t in c.tiles}) == 2:
        p.add("transposed+plain")
    for t in c.tiles:
        p |= {"k_valid:%d" % t[1], "p_valid:%d" % t[3]}
        if t[0] + TT > c.x2_off:
            p.add("window past the piece")
    return p


TG_PATHS = ({"PT:128", "PT:192", "tiles:1", "tiles:16", "transposed+plain", "window past the piece", "regime:exact", "regime:seeded", "splits:1", "splits:2",
             "splits:16", "splits:38"} | {"k_valid:%d" % v for v in (1, 127, 128, 129, 191, 192)} | {"p_valid:%d" % v for v in (1, 127, 128, 129, 191, 192)})


# ------------------------------------------------------------------------------------------------ encoders
def encode(x, s):
    """-> (h1, 2^11 h2, h2, 2^-11 h1) as fp16 of the fp32 matrix x under the scale s"""
    x = np.asarray(x, dtype=F32)
    with np.errstate(all="ignore"):
        v = x * F32(s)
        h1 = v.astype(F16)
        r = (x.astype(F64) * float(F32(s)) - h1.astype(F64)).astype(F32)        # fma(x, s, -h1): one rounding
        return h1, (r * F32(SHIFT)).astype(F16), r.astype(F16), (h1.astype(F32) * F32(1.0 / SHIFT)).astype(F16)


def scale_of(m):
    """halves_scale from max|x| = m (NaNs dropped before): s = 2^min(60, 14 - ceil(log2 m)); 1 for m = 0 or infinite"""
    s = 1.0
    if m > 0.0 and math.isfinite(m):
        f, e = math.frexp(float(F32(m)))
        if f == 0.5:
            e -= 1
        s = 2.0 ** min(60, 14 - e)
    return np.array([s, F32(1.0) / F32(s)], dtype=F32)


def absmax_of(x):
    a = np.abs(np.asarray(x, dtype=F32))
    a = a[~np.isnan(a)]
    return float(a.max()) if a.size else 0.0


def split_expected(x, s, order, piece, out, width=None, col=0, mutant=None):
    """bot_halves_split_f16 / _cols_f16 into `out` [n, ldo] (modified in place, a copy of what the buffer held before): `width` columns from
    `col` of every piece, F of them from x and zeros behind.  mutant "stale_padding": the zeros of the last block are not written."""
    n, F = x.shape
    width = piece if width is None else width
    h1, h2s, h2, h1s = encode(x, s)
    pieces = {0: (h1, h1, h2s), 1: (h1, h2, h1s), 2: (h1, h2s)}[order]
    for k, h in enumerate(pieces):
        if mutant != "stale_padding":
            out[:, k * piece + col + F:k * piece + col + width] = 0
        out[:, k * piece + col:k * piece + col + F] = h
    return out


def heads_expected(x, s, H, D, DP, h2_off, out):
    h1, h2s, _, _ = encode(x, s)
    for h in range(H):
        out[:, h * DP:(h + 1) * DP] = 0
        out[:, h2_off + h * DP:h2_off + (h + 1) * DP] = 0
        out[:, h * DP:h * DP + D] = h1[:, h * D:(h + 1) * D]
        out[:, h2_off + h * DP:h2_off + h * DP + D] = h2s[:, h * D:(h + 1) * D]
    return out


def frag_expected(x, s, piece):
    n, F = x.shape
    h1, _, h2, _ = encode(x, s)
    b1, b2 = np.zeros((n, piece), F16), np.zeros((n, piece), F16)
    b1[:, :F], b2[:, :F] = h1, h2
    return frag_pack(b1, b2, F16(0))


def tail_expected(segments, s, h2_off, out):
    for (col, width, src) in segments:
        if src is None:
            out[:, col:col + width] = 0
            out[:, h2_off + col:h2_off + col + width] = 0
        else:
            h1, h2s, _, _ = encode(src, s)
            out[:, col:col + width], out[:, h2_off + col:h2_off + col + width] = h1, h2s
    return out


def tn_combine_reference(a, b, P, rem_a=None, rem_b=None):
    """float64; -> (value, sum of |terms|, number of terms)"""
    PP = a.shape[2] // 2
    a, b = a.astype(F64), b.astype(F64)
    s1, s2, s3 = a[:, :, :P].sum(0), a[:, :, PP:PP + P].sum(0), b[:, :, :P].sum(0)
    ab = np.abs(a[:, :, :P]).sum(0) + (np.abs(a[:, :, PP:PP + P]).sum(0) + np.abs(b[:, :, :P]).sum(0)) / SHIFT
    if rem_a is not None:
        ra, rb = rem_a.astype(F64), rem_b.astype(F64)
        s1, s2, s3 = s1 + ra[:, :P], s2 + ra[:, PP:PP + P], s3 + rb[:, :P]
        ab = ab + np.abs(ra[:, :P]) + (np.abs(ra[:, PP:PP + P]) + np.abs(rb[:, :P])) / SHIFT
    return s1 + (s2 + s3) / SHIFT, ab, a.shape[0] + (rem_a is not None)


def edge_values(rng, shape, big=False):
    """fp32 test data with the edges in it: 0, -0, fp32 subnormals, values whose product with the scale lands at fp16's overflow threshold
    and subnormal range, +-inf and NaN (big: the non-finite ones and the huge ones left out, for maxima that must stay finite)"""
    x = (rng.standard_normal(shape) * 10.0 ** rng.integers(-6, 3, size=shape)).astype(F32)
    flat = x.reshape(-1)
    edges = [0.0, -0.0, 1e-40, -3e-42, 2.0 ** -126, 65504.0, -65520.0, 65519.99, 2.0 ** -24, 2.0 ** -25, 3 * 2.0 ** -26, 1.0 + 2.0 ** -11, 1.0 + 2.0 ** -10,
             2049.0, 4098.0]
    if not big:
        edges += [float("inf"), float("-inf"), float("nan"), 3e38, -1e30]
    pos = rng.permutation(flat.size)[:len(edges)]
    for p, e in zip(pos, edges[:len(pos)]):
        flat[p] = F32(e)
    return x


ENC_N = (1, 15, 16, 17, 4099)
ENC_F = (1, 63, 64, 65, 250, 750)


def encoder_cases():
    """(n, F, x row pitch - F, x base offset in floats, scale exponent or None for halves_scale's own)"""
    L = []
    for i, F in enumerate(ENC_F):
        n = ENC_N[i % len(ENC_N)]
        L.append((n, F, (0, 1, 2, 3)[i % 4], (0, 2, 1)[i % 3], (3, 0, -20, 60, 12, None)[i % 6]))
    for i, n in enumerate(ENC_N):
        L.append((n, (250, 65, 750, 1, 64)[i], (2, 0, 0, 5, 0)[i], (2, 0, 1, 0, 0)[i], (None, 5, -114, 3, 60)[i]))
    return L


# ------------------------------------------------------------------------------------------------ coverage
def cases():
    return [("nt", c) for c in nt_cases()] + [("nt_grouped", c) for c in ng_cases()] + [("tn", c) for c in tn_cases()] + [("tn_grouped", c) for c in tg_cases()]


def expected_kernels(kind, c):
    """every kernel name the GPU test must see for this case"""
    if kind == "nt":
        names = [expected_nt(c.K, mode, int(c.frag)) for mode in nt_modes(c)]
        if c.bn:
            names += [expected_nt(c.K, 0, int(c.frag), bn) for bn in ("store", "reduce", "apply")]
        return names
    if kind == "nt_grouped":
        return [expected_nt_grouped(c.groups, c.k_seg, c.mode, c.stats)]
    if kind == "tn":
        return [expected_tn()]
    return [expected_tn_grouped(c.tiles)]


def assert_coverage():
    """cases() reaches every launch form and every internal path the case lists promise -> the number of cases"""
    seen, paths = set(), {"nt": set(), "nt_grouped": set(), "tn": set(), "tn_grouped": set()}
    fn = {"nt": nt_paths, "nt_grouped": ng_paths, "tn": tn_paths, "tn_grouped": tg_paths}
    for kind, c in cases():
        names = expected_kernels(kind, c)
        assert None not in names, (kind, c)
        seen |= set(names)
        paths[kind] |= fn[kind](c)
    assert seen == all_forms(), (all_forms() - seen, seen - all_forms())
    for kind, want in (("nt", NT_PATHS), ("nt_grouped", NG_PATHS), ("tn", TN_PATHS), ("tn_grouped", TG_PATHS)):
        assert want <= paths[kind], (kind, sorted(want - paths[kind]))
    return len(cases())


def assert_exact(kind, o):
    """the exact regime's premise for one case, checked entry by entry in float64"""
    if kind == "nt":
        exact_premise(nt_reference(o), nt_quantum(o))
    elif kind == "nt_grouped":
        r = ng_reference(o)
        w = r["written"]
        alpha = float(o.sa[1]) * float(o.sb[1])
        q = 2.0 ** -11 * alpha * (0.5 if o.cs is not None else 1.0)
        cs = np.ones(o.c.width) if o.cs is None else np.abs(o.cs.astype(F64))
        ch = np.zeros(o.c.width) if o.ch is None else np.abs(o.ch.astype(F64))
        total = (r["ab"] * cs + ch)[w]
        assert float(total.max()) / q < 2.0 ** 24
        v = r["val"][w]
        assert np.array_equal(v.astype(F32).astype(F64), v) and np.array_equal(v, np.round(v / q) * q)
    elif kind == "tn":
        exact_premise(tn_reference(o), 2.0 ** -11 * tn_alpha(o)[None, :])
    else:
        val, s, w = tg_reference(o)
        q = 2.0 ** -11 * float(o.sx[1]) * float(o.sd[1])
        assert float(s.ab[w].max()) / q < 2.0 ** 24
        assert np.array_equal(val[w].astype(F32).astype(F64), val[w]) and np.array_equal(val[w], np.round(val[w] / q) * q)
