"""tests/halves_cases.py held to account on the CPU: the float64 restatements of the halves GEMMs against a plain float64 matmul of the
DECODED operands ((h1 + h2 / 2^11) / s, minus the term the format drops) and against the float32 emulation the CPU suite runs in place of
the kernels (tests/_oracle_backend.py); the restated dispatch, split counts and routes; the premise of the exact regime for every case;
twelve mutants of the restatements, each of which must change bits in the exact regime and exceed the derived bound in the seeded one; and
every argument check of the five C entry points, one bad argument at a time (they return before any launch)."""
import ctypes

import numpy as np
import pytest
import torch

from bot_amd import _C, gemm
from tests import _oracle_backend as OB
from tests import halves_cases as HC

F16, F32, F64 = np.float16, np.float32, np.float64
LONG = 100000          # rows


def _t(a):
    return torch.from_numpy(a)


def _ids(cases):
    return ["%s-%d-%s" % ("_".join(w for w in "".join(ch if ch.isalnum() else " " for ch in c.tag).split()), c.seed, c.regime) for c in cases]


# ------------------------------------------------------------------------------------------------ 1. a second way to the same number
@pytest.mark.parametrize("c", HC.nt_cases(), ids=_ids(HC.nt_cases()))
def test_nt_restatement_against_float64_matmul_and_the_emulation(c):
    o = HC.make_nt(c)
    s = HC.nt_reference(o)
    a1, a2, b1, b2 = (t.astype(F64) for t in HC.nt_pieces(o))
    sa = np.full(c.K, float(o.sa[0]))
    if c.k_split:
        sa[c.k_split:] = float(o.sa2[0])
    A, B = (a1 + a2 / HC.SHIFT) / sa, (b1 + b2) / float(o.sb[0])
    dropped = ((a2 / HC.SHIFT) / sa) @ (b2 / float(o.sb[0])).T
    # the third factor is ROUNDED where 2^-11 b1 is an fp16 subnormal: the decoded product does not round
    slack = (np.abs(a2) / sa) @ np.abs(HC.shifted(b1).astype(F64) - b1 / HC.SHIFT).T / float(o.sb[0])
    assert np.all(np.abs(A @ B.T - dropped - s.val) <= 1e-12 * s.ab + slack * (1 + 1e-12))
    if c.regime == "exact":
        assert float(slack.max()) == 0.0
        HC.exact_premise(s, HC.nt_quantum(o))
    # the float32 emulation of the CPU suite
    kw = dict(a2_off=o.a2_off, b_frag=c.frag, n=c.n)
    if c.k_split:
        kw.update(scale_a2=_t(o.sa2), k_split=c.k_split)
    got = OB.gemm_halves3_nt(_t(o.A), _t(o.B).reshape(-1, 512) if c.frag else _t(o.B), _t(o.sa), _t(o.sb), c.K, c.K if c.frag else o.b2_off, c.K, **kw).numpy()
    if c.regime == "seeded":
        assert np.all(np.abs(got.astype(F64) - s.val) <= HC.seeded_bound(s, 1))
    else:
        assert HC.same_bits(got + F32(0), s.val.astype(F32)).all()       # (+ 0: the emulation's BLAS may return -0 for a sum of zero products)


@pytest.mark.parametrize("c", HC.tn_cases(), ids=_ids(HC.tn_cases()))
def test_tn_restatement_against_float64_matmul_and_the_emulation(c):
    o = HC.make_tn(c)
    s = HC.tn_reference(o)
    x1, x2 = o.X[:, :c.K].astype(F64), o.X[:, o.x2_off:o.x2_off + c.K].astype(F64)
    d1, d2 = o.D[:, :c.P].astype(F64), o.D[:, o.d2_off:o.d2_off + c.P].astype(F64)
    sd = np.full(c.P, float(o.sd[0]))
    if c.p_split:
        sd[c.p_split:] = float(o.sd2[0])
    sx = float(o.sx[0])
    X, D = (x1 + x2 / HC.SHIFT) / sx, (d1 + d2 / HC.SHIFT) / sd
    dropped = (x2 / HC.SHIFT / sx).T @ (d2 / HC.SHIFT / sd)
    slack = (np.abs(HC.shifted(x1).astype(F64) - x1 / HC.SHIFT) / sx).T @ (np.abs(d2) / sd) + (np.abs(x2) / sx).T @ (np.abs(HC.shifted(d1).astype(F64) - d1 / HC.SHIFT) / sd)
    assert np.all(np.abs(X.T @ D - dropped - s.val) <= 1e-12 * s.ab + slack * (1 + 1e-12))
    if c.regime == "exact":
        assert float(slack.max()) == 0.0
    kw = dict(x2_off=o.x2_off, d2_off=o.d2_off)
    if c.p_split:
        kw.update(scale_d2=_t(o.sd2), p_split=c.p_split)
    got = OB.gemm_halves3_tn(_t(o.X), _t(o.D), _t(o.sx), _t(o.sd), o.kp, o.pp, c.K, c.P, **kw).numpy()
    if c.regime == "seeded":
        assert np.all(np.abs(got.astype(F64) - s.val) <= HC.seeded_bound(s, 1))
    else:
        assert HC.same_bits(got + F32(0), s.val.astype(F32)).all()       # (+ 0: the emulation's BLAS may return -0 for a sum of zero products)


@pytest.mark.parametrize("c", HC.ng_cases(), ids=_ids(HC.ng_cases()))
def test_nt_grouped_restatement_against_the_emulation(c):
    """the emulation accumulates in the output's type: float64 here, so it IS a second float64 evaluation of the header's formula"""
    o = HC.make_ng(c)
    r = HC.ng_reference(o)
    out = torch.full((c.m, c.width), float("nan"), dtype=torch.float64)
    slots = OB.absmax_slots("cpu")
    tiles = (c.m + 255) // 256
    stats = tuple(torch.full(s, float("nan")) for s in ((tiles, 2, c.width), (tiles, 2, c.width), (tiles, c.width))) if c.stats else None
    OB.gemm_halves3_nt_grouped(_t(o.A), _t(o.B), _t(o.sa), _t(o.sb), c.a2_off, c.b2_off, out, [list(g) for g in c.groups], c.k_seg,
                               col_scale=None if o.cs is None else _t(o.cs), col_shift=None if o.ch is None else _t(o.ch), relu=c.relu, absmax=slots, stats=stats)
    got, w = out.numpy(), r["written"]
    assert np.array_equal(np.isnan(got), ~w)
    tol = 1e-12 * (np.abs(r["val"][w]) + r["bound"][w] / HC.U * 1e-3)
    assert np.all(np.abs(got[w] - r["val"][w]) <= tol + 1e-300)
    assert float(slots.max().reshape(1).view(torch.float32)[0]) == float(F32(r["absmax"]))
    if c.stats:
        st = HC.stored_stats(got.astype(F32), w, c.m)
        part, minmax, pivot = (t.numpy() for t in stats)
        col = w[0]
        assert np.array_equal(pivot[:, col], st["pivot"][:, col].astype(F32)) and np.array_equal(minmax[:, 0][:, col], st["min"][:, col].astype(F32))
        assert np.array_equal(minmax[:, 1][:, col], st["max"][:, col].astype(F32))
        wide = 300 * HC.U            # the emulation's float32 column sums: at most one rounding per row on any path
        assert np.all(np.abs(part[:, 0][:, col] - st["sum"][:, col]) <= wide * st["a_sum"][:, col] + 1e-30)
        assert np.all(np.abs(part[:, 1][:, col] - st["sumsq"][:, col]) <= wide * st["a_sumsq"][:, col] + 1e-30)
    if c.regime == "exact":
        HC.assert_exact("nt_grouped", o)


@pytest.mark.parametrize("c", HC.tg_cases(), ids=_ids(HC.tg_cases()))
def test_tn_grouped_restatement_against_the_emulation(c):
    o = HC.make_tg(c)
    val, s, w = HC.tg_reference(o)
    out = torch.full((c.out_floats,), float("nan"), dtype=torch.float64)
    OB.gemm_halves3_tn_grouped(_t(o.X), _t(o.D), _t(o.sx), _t(o.sd), c.x2_off, c.d2_off, out, [list(t) for t in c.tiles])
    got = out.numpy()
    assert np.array_equal(np.isnan(got), ~w)
    assert np.all(np.abs(got[w] - val[w]) <= 1e-12 * s.ab[w])
    if c.regime == "exact":
        HC.assert_exact("tn_grouped", o)


def test_exact_premise_of_the_long_cases_and_coverage():
    n = HC.assert_coverage()
    assert n == len(HC.cases()) and len(HC.all_forms()) == 16
    for c in HC.tn_cases():
        if c.regime == "exact":
            HC.assert_exact("tn", HC.make_tn(c))
        elif c.n >= LONG:                  # the long seeded reduction keeps a tight bound because it is sparse
            s = HC.tn_reference(HC.make_tn(c))
            assert float(s.nz.max()) < 4000 and float(HC.gamma(2 * s.nz.max() + 66)) < 1e-3


# ------------------------------------------------------------------------------------------------ 2. dispatch, splits, routes
def test_dispatch_by_hand():
    N, T = HC.NT_FORMS, HC.TN_FORMS
    assert HC.expected_kernel("nt", 64) == N["nt64"] and HC.expected_kernel("tn") == T["tn"] and HC.expected_nt(96) == N["nt_pipelined"] and HC.expected_nt(32) == N["nt_pipelined"]
    assert HC.expected_nt(128, HC.MODE_128X64) == N["nt_pipelined"] and HC.expected_nt(128, HC.MODE_PLAIN) == N["nt_plain"]
    assert HC.expected_nt(128, HC.MODE_ABLATE) == N["nt_ablate"] and HC.expected_nt(128, 0, 1) == N["nt64_frag"]
    assert HC.expected_nt(96, 0, 1) is None and HC.expected_nt(128, HC.MODE_128X64, 1) is None and HC.expected_nt(128, HC.MODE_PLAIN, 1) is None
    assert HC.expected_nt(128, 0, 0, "store") == N["nt64_bnb"] and HC.expected_nt(128, 0, 1, "apply") == N["nt64_frag_bnapply"]
    assert HC.expected_nt(96, 0, 0, "reduce") is None and HC.expected_nt(64, 0, 1, "reduce") == N["nt64_frag_bnreduce"]
    assert HC.expected_nt_grouped([(0, 1, 0, 0, 2, 0)], 0) == N["nt64_grouped"] and HC.expected_nt_grouped([(0, 1, 0, 0, 3, 0)], 0) == N["nt_grouped"]
    assert HC.expected_nt_grouped([(0, 1, 0, 0, 2, 0)], 1) == N["nt_grouped"] and HC.expected_nt_grouped([(0, 1, 0, 0, 2, 0)], 1, stats=True) is None
    assert HC.expected_tn_grouped([(0, 1, 0, 128, 0, 128, 0)]) == T["tn_grouped128"] and HC.expected_tn_grouped([(0, 1, 0, 129, 0, 129, 0)]) == T["tn_grouped192"]
    assert _C._lib.bot_gemm_halves3_nt_bn_rows(128) == 256 and _C._lib.bot_gemm_halves3_nt_bn_rows(96) == 0


def test_split_counts_against_the_workspace_functions():
    """tn_splits / tn_grouped_splits, restated, against bot_gemm_halves3_tn{,_grouped}_workspace_floats (host functions)"""
    for n in (1, 31, 32, 33, 4095, 4096, 8191, 8192, 8193, 32767, 32768, 32773, 65536, 169343, 262149, 1 << 20):
        for (kp, pp) in ((64, 64), (192, 192), (256, 64), (768, 1536), (512, 1024), (448, 192)):
            s, launched, rps = HC.tn_splits(n, kp, pp)
            assert _C._lib.bot_gemm_halves3_tn_workspace_floats(n, kp, pp) == s * kp * pp, (n, kp, pp)
            assert 1 <= launched <= s and rps % 32 == 0 and (launched - 1) * rps < n <= launched * rps
    assert [HC.tn_splits(n, 64, 64)[0] for n in (1, 4095, 8192, 8193, 32773, 262149)] == [1, 1, 2, 2, 8, 64]
    assert HC.tn_splits(169343, 768, 1536)[0] == 8 and HC.tn_splits(1 << 20, 576, 1152)[0] == 56      # 18 tiles: q = 7
    for n in (1, 1023, 1024, 2047, 2049, 40000, 169343):
        for t in (1, 2, 3, 8, 12, 16):
            s, launched, rps = HC.tn_grouped_splits(n, t)
            assert _C._lib.bot_gemm_halves3_tn_grouped_workspace_floats(n, t) == s * t * 192 * 192
            assert 1 <= launched <= s and (launched - 1) * rps < n <= launched * rps
    assert HC.tn_grouped_splits(40000, 3)[:2] == (39, 38) and HC.tn_grouped_splits(40000, 16)[:2] == (16, 16)


def test_routes_of_gemm_py(monkeypatch):
    """gemm.left_order / split_right / _tn_tiles and the predicates of mm_nt / tn against their restatement, at the thresholds"""
    OB.install(monkeypatch)
    monkeypatch.setattr(gemm, "FORCE", True)
    kw = dict(nodup=gemm.LEFT_NODUP, min_piece=gemm.NODUP_MIN_PIECE)
    for piece in (64, 192, 256, 320):
        assert gemm.left_order(piece) == HC.left_order(piece, **kw)
    assert HC.left_order(192, **kw) == 0 and HC.left_order(256, **kw) == 2
    for (p, F) in ((191, 100), (192, 100), (40, 192), (40, 193), (40, 256), (191, 250)):
        w = torch.randn(p, F)
        assert gemm.split_right(w).order == HC.split_right_order(p, F, gemm.RIGHT_FRAG, gemm.NT_MIN_COLS, **kw), (p, F)
        assert gemm.split(torch.randn(5, F), 0).order == HC.left_order(HC.piece_of(F), **kw)
    assert HC.split_right_order(191, 100) == 1 and HC.split_right_order(192, 100) == 3 and HC.split_right_order(40, 193) == 3
    for (K, P) in ((750, 240), (100, 968), (64, 40), (1536, 750), (3000, 192), (3073, 192), (3072, 193)):
        assert gemm._tn_tiles(K, P) == HC.tn_tiles(K, P)
    assert len(HC.tn_tiles(3072, 128)) == 16 and HC.tn_tiles(3073, 128) is None          # a tile grid of 16 and one of 17
    assert HC.tn_route(8192, 512, 1024) == HC.TN_FORMS["tn"] and HC.tn_route(8192, 512, 960) == HC.TN_FORMS["tn_grouped192"]           # KP PP = 2^19 and below
    assert HC.tn_route(8192, 512, 896) == HC.TN_FORMS["tn_grouped192"] and HC.tn_route(8191, 512, 896) == "lib"
    assert HC.tn_route(8192, 750, 240) == HC.TN_FORMS["tn_grouped128"] and HC.tn_route(8192, 3073, 128) == "lib"
    assert HC.mm_nt_route(0, 1, 191, 192) == "lib" and HC.mm_nt_route(0, 1, 192, 192) == HC.NT_FORMS["nt64"]
    assert HC.mm_nt_route(2, 1, 40, 256) == HC.NT_FORMS["nt64"] and HC.mm_nt_route(0, 3, 40, 192) == HC.NT_FORMS["nt64_frag"]
    assert HC.mm_nt_route(0, 1, 300, 96) == HC.NT_FORMS["nt_pipelined"]
    assert gemm.TN_MIN_OUT == 512 * 1024 and gemm.NT_MIN_COLS == 192 and gemm.NODUP_MIN_PIECE == 256 and gemm.MIN_ROWS == 8192


# ------------------------------------------------------------------------------------------------ 3. encoders
def test_encoder_restatement_against_the_emulation_and_the_format():
    rng = np.random.default_rng(5)
    for (n, F, pad, off, e) in HC.encoder_cases():
        if n > 100:
            continue
        x = HC.edge_values(rng, (n, F), big=True)
        sc = HC.scale_of(HC.absmax_of(x)) if e is None else HC.pow2(e)
        assert np.array_equal(sc, OB.halves_scale(_t(x)).numpy()) or e is not None
        h1, h2s, h2, h1s = HC.encode(x, sc[0])
        piece = HC.piece_of(F)
        for order in (0, 1, 2):
            want = HC.split_expected(x, sc[0], order, piece, np.full((n, (2 if order == 2 else 3) * piece), HC.NAN16, F16))
            got = OB.halves_split(_t(x), _t(sc), order, piece).numpy()
            # (+ 0: where x s underflows in float32 the emulation's v - h1 is +0 and the kernel's fma(x, s, -h1) keeps the sign)
            assert HC.same_bits(got + F16(0), want + F16(0)).all(), (n, F, order)
        # the format's promise (the existing property): (h1 + h2) / s reproduces x to 2^-22 of the largest entry
        if e is None:
            dec = (h1.astype(F64) + h2s.astype(F64) / HC.SHIFT) / float(sc[0])
            assert float(np.abs(dec - x.astype(F64)).max()) <= 2.0 ** -22 * HC.absmax_of(x)
        assert HC.same_bits(HC.frag_expected(x, sc[0], piece).reshape(-1, 512) + F16(0), OB.halves_split_frag(_t(x), _t(sc), piece).numpy() + F16(0)).all()
    # the exponent clamps of halves_scale and its special inputs
    assert HC.scale_of(0.0)[0] == 1.0 and HC.scale_of(float("inf"))[0] == 1.0 and HC.scale_of(1e-30)[0] == 2.0 ** 60
    assert HC.scale_of(1.0)[0] == 2.0 ** 14 and HC.scale_of(1.0 + 2.0 ** -23)[0] == 2.0 ** 13 and HC.scale_of(3e38)[0] == 2.0 ** -114
    assert np.isfinite(HC.scale_of(3e38)[1]) and HC.scale_of(2.0 ** -149)[0] == 2.0 ** 60
    # the fragment-major index is a bijection onto the buffer
    for (n, piece) in ((1, 64), (17, 64), (250, 192)):
        idx, region = HC.frag_index(n, piece)
        assert np.array_equal(np.sort(idx.reshape(-1)), np.arange(region))


# ------------------------------------------------------------------------------------------------ 4. mutants
def _differs(ref, mut, bound, exact):
    """what test_halves_gpu.py would see if the device returned `mut` where `ref` is right"""
    with np.errstate(all="ignore"):
        if exact:
            return not HC.same_bits(np.nan_to_num(mut, nan=-7.0).astype(F32), np.nan_to_num(ref, nan=-7.0).astype(F32)).all()
        return bool(np.any(np.nan_to_num(np.abs(mut - ref), nan=np.inf) > np.nan_to_num(bound, nan=0.0)))


def _first(cases, **kw):
    return next(c for c in cases if all(getattr(c, k) == v for k, v in kw.items()))


@pytest.mark.parametrize("regime", ("exact", "seeded"))
@pytest.mark.parametrize("mutant", HC.NT_MUTANTS + HC.NG_MUTANTS + HC.TN_MUTANTS[:1] + HC.TG_MUTANTS + ("stale_padding",))
def test_mutants_are_caught_in_both_regimes(mutant, regime):
    exact = regime == "exact"
    if mutant in HC.NT_MUTANTS:
        two = mutant in ("rescale_late", "alpha_from_scale_a")
        c = next(c for c in HC.nt_cases() if c.regime == regime and bool(c.k_split) == two and c.K >= 128 and (not two or c.k_split < c.K - 32))
        o = HC.make_nt(c)
        ref, mut = HC.nt_reference(o), HC.nt_reference(o, mutant)
        assert _differs(ref.val, mut.val, HC.seeded_bound(ref, 1), exact), (mutant, c)
    elif mutant in HC.NG_MUTANTS:
        c = next(c for c in HC.ng_cases() if c.regime == regime and c.k_seg and len(c.groups) == 2 and (c.stats or mutant != "stats_with_clamped_rows"))
        o = HC.make_ng(c)
        ref, mut = HC.ng_reference(o), HC.ng_reference(o, mutant)
        if mutant == "stats_with_clamped_rows":
            assert c.m % 256 > 1
            st = HC.stored_stats(ref["val"].astype(F32), ref["written"], c.m)
            for k, e in (("sum", "e_sum"), ("sumsq", "e_sumsq")):
                assert _differs(st[k], mut[k], st[e], False), (mutant, k)
        else:
            assert _differs(ref["val"], mut["val"], ref["bound"], exact), (mutant, c)
    elif mutant == "p_split_one_quad_late":
        c = next(c for c in HC.tn_cases() if c.regime == regime and c.p_split)
        o = HC.make_tn(c)
        ref, mut = HC.tn_reference(o), HC.tn_reference(o, mutant)
        assert _differs(ref.val, mut.val, HC.seeded_bound(ref, 1), exact)
    elif mutant == "ignore_transposed":
        c = next(c for c in HC.tg_cases() if c.regime == regime and any(t[6] for t in c.tiles))
        o = HC.make_tg(c)
        (ref, s, _), (mut, _, _) = HC.tg_reference(o), HC.tg_reference(o, mutant)
        assert _differs(ref, mut, HC.seeded_bound(s, 1), exact)
    else:        # the encoders are bit for bit in every regime: the last block's zero padding left stale
        rng = np.random.default_rng(3)
        x = HC.edge_values(rng, (5, 7)) if exact else rng.standard_normal((5, 7)).astype(F32)
        buf = np.full((5, 3 * 64), HC.NAN16, F16)
        a = HC.split_expected(x, 4.0, 0, 64, buf.copy(), width=10, col=20)
        b = HC.split_expected(x, 4.0, 0, 64, buf.copy(), width=10, col=20, mutant=mutant)
        assert not HC.same_bits(a, b).all() and HC.same_bits(a[:, 20:27], b[:, 20:27]).all()


def test_the_checks_accept_the_restatement_itself():
    for kind, c in HC.cases():
        if kind == "nt" and c.tag in ("K", "k_split") and c.m * c.n < 20000:
            o = HC.make_nt(c)
            ref = HC.nt_reference(o)
            assert not _differs(ref.val, ref.val.astype(F32).astype(F64), HC.seeded_bound(ref, 1), c.regime != "seeded")


# ------------------------------------------------------------------------------------------------ 5. the argument checks, no launch
_MEM = torch.zeros(1 << 16, dtype=torch.float32)
_PTR = _MEM.data_ptr()


def _bn(**kw):
    a = dict(x=_PTR, ldx=4, mean=_PTR, invstd=_PTR, weight=None, bias=None, relu=0, p=0.0, seed=1, seed_offset=None, part=_PTR, pmax=None)
    a.update(kw)
    return _C._BnBwdStats(*a.values())


def _nt3(**kw):
    a = dict(m=4, n=4, k=64, scale_a=_PTR, scale_a2=None, k_split=0, scale_b=_PTR, A=_PTR, lda=192, a2_off=128, B=_PTR, ldb=128, b2_off=64, b_layout=0, C=_PTR,
             ldc=4, bn=None, mode=0, stream=None)
    a.update(kw)
    if a["bn"] is not None:
        a["_keep"] = a["bn"]
        a["bn"] = ctypes.addressof(a["bn"])
    return _C._lib.bot_gemm_halves3_nt3_f32(*[v for k, v in a.items() if k != "_keep"])


def _ng(**kw):
    g = kw.pop("group", (0, 4, 0, 0, 2, 0))
    tab = _C._table([g], 6)
    a = dict(m=4, b_rows=8, scale_a=_PTR, scale_b=_PTR, A=_PTR, lda=192, a2_off=96, B=_PTR, ldb=192, b2_off=96, C=_PTR, ldc=4, n_groups=1,
             groups=ctypes.addressof(tab), k_seg=0, col_scale=None, col_shift=None, relu=0, absmax=None, sp=None, sm=None, sv=None, sF=0, mode=0, stream=None)
    a.update(kw)
    return _C._lib.bot_gemm_halves3_nt_grouped2_f32(*a.values())


def _tn2(**kw):
    a = dict(n_rows=40, k=60, p=60, kp=64, pp=64, scale_x=_PTR, scale_d=_PTR, scale_d2=None, p_split=0, X=_PTR, ldx=128, x2_off=64, D=_PTR, ldd=128, d2_off=64,
             out=_PTR, ldo=60, workspace=_PTR, mode=0, stream=None)
    a.update(kw)
    return _C._lib.bot_gemm_halves3_tn2_f32(*a.values())


def _tg(**kw):
    t = kw.pop("tile", (0, 60, 0, 60, 0, 60, 0))
    tab = _C._table([t], 7)
    a = dict(n_rows=40, scale_x=_PTR, scale_d=_PTR, X=_PTR, ldx=128, x2_off=64, D=_PTR, ldd=128, d2_off=64, out=_PTR, n_tiles=1, tiles=ctypes.addressof(tab),
             workspace=_PTR, mode=0, stream=None)
    a.update(kw)
    return _C._lib.bot_gemm_halves3_tn_grouped_f32(*a.values())


_BAD = [
    (_nt3, dict(k=40)), (_nt3, dict(k=0)), (_nt3, dict(m=0)), (_nt3, dict(n=0)), (_nt3, dict(scale_a=None)), (_nt3, dict(scale_b=None)), (_nt3, dict(A=None)),
    (_nt3, dict(B=None)), (_nt3, dict(C=None)), (_nt3, dict(A=_PTR + 2)), (_nt3, dict(B=_PTR + 8)), (_nt3, dict(lda=196)), (_nt3, dict(ldb=132)),
    (_nt3, dict(a2_off=132, lda=200)), (_nt3, dict(b2_off=68, ldb=136)), (_nt3, dict(lda=184)), (_nt3, dict(ldb=120)), (_nt3, dict(ldc=3)),
    (_nt3, dict(m=(1 << 31) - 256)), (_nt3, dict(scale_a2=_PTR, k_split=0)), (_nt3, dict(scale_a2=_PTR, k_split=64)), (_nt3, dict(scale_a2=_PTR, k_split=48)),
    (_nt3, dict(b_layout=2)), (_nt3, dict(b_layout=1, mode=32)), (_nt3, dict(b_layout=1, k=96, lda=224, ldb=192, b2_off=96)),
    (_nt3, dict(b_layout=1, mode=1024)), (_nt3, dict(bn=_bn(), mode=32)), (_nt3, dict(bn=_bn(), k=96, lda=224, ldb=192, b2_off=96)), (_nt3, dict(bn=_bn(x=None))),
    (_nt3, dict(bn=_bn(mean=None))), (_nt3, dict(bn=_bn(invstd=None))), (_nt3, dict(bn=_bn(part=None))), (_nt3, dict(bn=_bn(), n=3, ldc=4)),
    (_nt3, dict(bn=_bn(ldx=2))), (_nt3, dict(bn=_bn(ldx=5))), (_nt3, dict(bn=_bn(x=_PTR + 4))), (_nt3, dict(bn=_bn(p=1.0))), (_nt3, dict(bn=_bn(p=-0.5))),
    (_ng, dict(sp=_PTR)), (_ng, dict(sp=_PTR, sm=_PTR, sv=_PTR, sF=0)), (_ng, dict(m=0)), (_ng, dict(b_rows=0)), (_ng, dict(n_groups=0)), (_ng, dict(n_groups=13)),
    (_ng, dict(k_seg=-1)), (_ng, dict(groups=None)), (_ng, dict(A=None)), (_ng, dict(C=None)), (_ng, dict(scale_b=None)), (_ng, dict(A=_PTR + 2)),
    (_ng, dict(lda=196)), (_ng, dict(b2_off=100)), (_ng, dict(lda=1 << 22)), (_ng, dict(group=(8, 4, 0, 0, 2, 0))), (_ng, dict(group=(-1, 4, 0, 0, 2, 0))),
    (_ng, dict(group=(0, 0, 0, 0, 2, 0))), (_ng, dict(group=(0, 257, 0, 0, 2, 0))), (_ng, dict(group=(0, 4, 0, 0, 0, 0))), (_ng, dict(group=(0, 4, 4, 0, 2, 0), k_seg=1)),
    (_ng, dict(group=(0, 4, 0, 4, 2, 0))), (_ng, dict(group=(0, 4, 0, 0, 2, -1))), (_ng, dict(group=(0, 4, 0, 40, 2, 0))), (_ng, dict(group=(0, 4, 72, 0, 2, 0), k_seg=1)),
    (_ng, dict(group=(0, 4, 0, 0, 4, 0))), (_ng, dict(ldb=152)), (_ng, dict(sp=_PTR, sm=_PTR, sv=_PTR, sF=4, k_seg=1)),
    (_ng, dict(sp=_PTR, sm=_PTR, sv=_PTR, sF=4, mode=1024)), (_ng, dict(sp=_PTR, sm=_PTR, sv=_PTR, sF=4, group=(0, 4, 0, 0, 3, 0))),
    (_tn2, dict(scale_d2=_PTR, p_split=0)), (_tn2, dict(scale_d2=_PTR, p_split=64)), (_tn2, dict(scale_d2=_PTR, p_split=6)), (_tn2, dict(n_rows=0)), (_tn2, dict(k=0)),
    (_tn2, dict(p=0)), (_tn2, dict(k=65)), (_tn2, dict(p=65)), (_tn2, dict(kp=96, ldx=160)), (_tn2, dict(pp=96, ldd=160)), (_tn2, dict(scale_x=None)),
    (_tn2, dict(scale_d=None)), (_tn2, dict(X=None)), (_tn2, dict(D=None)), (_tn2, dict(out=None)), (_tn2, dict(workspace=None)), (_tn2, dict(X=_PTR + 2)),
    (_tn2, dict(D=_PTR + 8)), (_tn2, dict(ldx=132)), (_tn2, dict(ldd=132)), (_tn2, dict(x2_off=68, ldx=136)), (_tn2, dict(d2_off=68, ldd=136)), (_tn2, dict(ldx=120)),
    (_tn2, dict(ldd=120)), (_tn2, dict(ldo=59)), (_tn2, dict(n_rows=(1 << 31) - 4096)), (_tn2, dict(n_rows=1 << 24, ldx=1 << 12, x2_off=64)),
    (_tg, dict(n_rows=0)), (_tg, dict(n_tiles=0)), (_tg, dict(n_tiles=17)), (_tg, dict(tiles=None)), (_tg, dict(X=None)), (_tg, dict(out=None)),
    (_tg, dict(workspace=None)), (_tg, dict(scale_d=None)), (_tg, dict(D=_PTR + 4)), (_tg, dict(ldx=132)), (_tg, dict(d2_off=68)), (_tg, dict(x2_off=128)),
    (_tg, dict(d2_off=128)), (_tg, dict(tile=(4, 60, 0, 60, 0, 60, 0))), (_tg, dict(tile=(0, 60, 4, 60, 0, 60, 0))), (_tg, dict(tile=(-8, 60, 0, 60, 0, 60, 0))),
    (_tg, dict(tile=(0, 0, 0, 60, 0, 60, 0))), (_tg, dict(tile=(0, 193, 0, 60, 0, 60, 0), ldx=512, x2_off=256)), (_tg, dict(tile=(0, 60, 0, 0, 0, 60, 0))),
    (_tg, dict(tile=(0, 60, 0, 193, 0, 193, 0), ldd=512, d2_off=256)), (_tg, dict(tile=(0, 60, 0, 60, -1, 60, 0))), (_tg, dict(tile=(0, 60, 0, 50, 0, 49, 0))),
    (_tg, dict(tile=(0, 60, 0, 50, 0, 59, 1))), (_tg, dict(tile=(8, 60, 0, 60, 0, 60, 0))), (_tg, dict(tile=(0, 60, 8, 60, 0, 60, 0))),
    (_tg, dict(n_rows=1 << 24, ldx=1 << 14)),
]


@pytest.mark.parametrize("i", range(len(_BAD)))
def test_argument_checks_refuse_one_bad_argument_at_a_time(i):
    fn, kw = _BAD[i]
    rc = fn(**kw)
    assert rc < 0 and _C._lib.bot_last_error(), (fn.__name__, kw, rc)          # (negative: a check's code; a launch error would be a positive HIP code)
    with pytest.raises(_C.BotKernelError):
        _C._check(rc, fn.__name__)


def test_deferred_pair_argument_checks():
    """bot_gemm_halves3_nt_bn_reduce_f32 / _apply_f32: their own conditions (BOT_E_NULL -1, BOT_E_RANGE -2), before the shared ones"""
    bn = _bn()
    base = [4, 4, 64, _PTR, None, 0, _PTR, _PTR, 192, 128, _PTR, 128, 64, 0]

    def reduce(bn_, k=64, n=4):
        a = list(base)
        a[1], a[2] = n, k
        return _C._lib.bot_gemm_halves3_nt_bn_reduce_f32(*a, None, 0, None if bn_ is None else ctypes.addressof(bn_), None)

    def apply(bn_, sum_g=None, sum_gx=None, total=4.0, dx=_PTR, lddx=4, hscale=None, hout=None, ldh=0, h2_off=0, hD=2, hDP=2):
        return _C._lib.bot_gemm_halves3_nt_bn_apply_f32(*base, ctypes.addressof(bn_), sum_g, sum_gx, total, dx, lddx, hscale, hout, ldh, h2_off, hD, hDP, None, None)
    assert reduce(None) == -1 and reduce(_bn(x=None)) == -1 and reduce(_bn(part=None)) == -1
    assert reduce(bn, k=320) == -2 and reduce(bn, k=96) == -2 and reduce(bn, n=3) == -2 and reduce(_bn(ldx=2)) == -2 and reduce(_bn(p=1.0)) == -2
    assert reduce(_bn(x=_PTR + 4)) == -2
    assert apply(bn, dx=None) == -1 and apply(bn, sum_g=_PTR) == -1 and apply(bn, sum_g=_PTR, sum_gx=_PTR, total=0.5) == -2
    assert apply(bn, lddx=3) == -2 and apply(bn, lddx=5) == -2 and apply(bn, dx=_PTR + 4) == -2 and apply(bn, hout=_PTR) == -1
    for kw in (dict(hD=1), dict(hD=3), dict(hDP=0), dict(hD=2, hDP=3), dict(hD=6), dict(h2_off=3, ldh=8), dict(h2_off=2, ldh=8), dict(h2_off=4, ldh=6), dict(h2_off=4, ldh=9)):
        a = dict(hscale=_PTR, hout=_PTR, ldh=8, h2_off=4, hD=2, hDP=2)
        a.update(kw)
        assert apply(bn, **a) == -2, kw
    assert _C._lib.bot_gemm_halves3_nt_bn_deferred_max_k() == 256
