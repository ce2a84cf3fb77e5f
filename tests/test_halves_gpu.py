"""The halves GEMMs (csrc/halves3.hip) and their encoders (csrc/halves.hip) on the MI355X against the float64 restatements of
tests/halves_cases.py, at every launch form: sixteen kernel names behind bot_gemm_halves3_nt{,2,3}_f32 (+ the deferred pair),
_nt_grouped{,2}_f32, _tn{,2}_f32 and _tn_grouped_f32.

Every case hands the kernel fp16 pieces that are independent of each other inside allocations whose every other element is NaN (guard rows,
the duplicate piece, rows of other groups, columns outside a tile's valid range); outputs are views into sentinel-filled allocations.  Exact
cases must come back bit for bit, seeded ones under the per-entry bound gamma(2 nnz + splits + 2) sum |terms| alpha with u = 2^-23; after
every launch bot_last_kernel() is the name the restated dispatch predicts, and the last test holds the set of names seen to all_forms()."""
import numpy as np
import pytest
import torch

from bot_amd import _C, gemm
from tests import halves_cases as HC
from tests import spmm_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda"
F16, F32, F64 = np.float16, np.float32, np.float64
SEEN = set()          # kernel names reported by bot_last_kernel()
RAN = set()           # the case lists that ran in this process
WORST = {}            # entry point -> largest observed error / bound of the seeded regime


def _ids(cases):
    return ["%s-%d-%s" % ("_".join(w for w in "".join(ch if ch.isalnum() else " " for ch in c.tag).split()), c.seed, c.regime) for c in cases]


def _last(expected):
    name = _C._lib.bot_last_kernel().decode()
    assert name == expected, (name, expected)
    SEEN.add(name)


def _up(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _rows(full, rows):
    """the operand's rows inside its uploaded allocation (guard rows before and behind)"""
    return _up(full)[HC.GUARD_ROWS:HC.GUARD_ROWS + rows]


def _flat16(flat):
    """a flat fp16 buffer between two NaN guards of 64 halves (the base stays 16-byte aligned)"""
    g = np.full(64, HC.NAN16, F16)
    return _up(np.concatenate([g, flat, g]))[64:64 + flat.size]


def _out(shape, pad=0, off=0):
    r = SC.Recipe(off=off, pad=pad)
    buf, view = SC.place_out(shape, r, DEV)
    return buf, view, r


def _check(entry, tag, got, s, exact, splits=1):
    """got (float32 numpy) against the restatement s (Sum3): bit for bit, or under the seeded bound (ratio recorded)"""
    if exact:
        bad = ~HC.same_bits(got, s.val.astype(F32))
        assert not bad.any(), (entry, tag, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], s.val[bad][:4])
        return
    bound = HC.seeded_bound(s, splits)
    err = np.abs(got.astype(F64) - s.val)
    ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    WORST[entry] = max(WORST.get(entry, 0.0), ratio)
    print(f"{entry} {tag}: worst error / bound {ratio:.3f}")
    assert ratio <= 1.0, (entry, tag, ratio)


# ------------------------------------------------------------------------------------------------ NT, plain
def _nt_operands(o):
    c = o.c
    a = _rows(o.afull, c.m)
    b = _flat16(o.B).view(-1, 512) if c.frag else _rows(o.bfull, c.n)
    return a, b, _up(o.sa), _up(o.sb), (_up(o.sa2) if c.k_split else None)


def _nt_kw(o):
    c = o.c
    return dict(a2_off=o.a2_off, scale_a2=None, k_split=c.k_split, b_frag=c.frag, n=c.n)


def _run_nt(o, ops, mode, pad, off):
    c = o.c
    a, b, sa, sb, sa2 = ops
    buf, view, r = _out((c.m, c.n), pad, off)
    kw = _nt_kw(o)
    kw["scale_a2"] = sa2
    _C.gemm_halves3_nt(a, b, sa, sb, c.K, c.K if c.frag else o.b2_off, c.K, out=view, mode=mode, **kw)
    _last(HC.expected_nt(c.K, mode, int(c.frag)))
    got = view.cpu().numpy()
    assert SC.guards_intact(buf, view, r), (c, mode)
    return got


@pytest.mark.parametrize("c", HC.nt_cases(), ids=_ids(HC.nt_cases()))
def test_nt(c):
    o = HC.make_nt(c)
    s = HC.nt_reference(o)
    exact = c.regime != "seeded"
    if exact:
        HC.exact_premise(s, HC.nt_quantum(o))
    ops = _nt_operands(o)
    for mode in HC.nt_modes(c):
        _check("nt", (c.tag, c.seed, mode), _run_nt(o, ops, mode, c.pad, c.off), s, exact)
    RAN.add("nt")
    if not c.bn:
        return
    # ---- the BatchNorm-backward forms: the storing launch's C is the product's bits, the reduce-only launch leaves the same partials and
    # stores nothing, and the apply launch with running statistics, mean 0, invstd 1, no affine, no ReLU, p = 0 writes dx = the product
    a, b, sa, sb, sa2 = ops
    kw = dict(_nt_kw(o), scale_a2=sa2)
    rng = np.random.default_rng(c.seed)
    x = _up(rng.standard_normal((c.m, c.n)).astype(F32))
    mean, invstd = _up(rng.standard_normal(c.n).astype(F32)), _up((rng.random(c.n) + 0.5).astype(F32))
    piece_b = c.K if c.frag else o.b2_off
    st = _C.BnBwdStats(x, mean, invstd, None, None, True, 0.5, 77)
    buf, view, r = _out((c.m, c.n), 2, 2)
    _C.gemm_halves3_nt(a, b, sa, sb, c.K, piece_b, c.K, out=view, bn=st, **kw)
    _last(HC.expected_nt(c.K, 0, int(c.frag), "store"))
    _check("nt", (c.tag, c.seed, "bnb"), view.cpu().numpy(), s, True)
    assert SC.guards_intact(buf, view, r)
    st2 = _C.BnBwdStats(x, mean, invstd, None, None, True, 0.5, 77)
    st2.part.fill_(7.0), st2.pmax.fill_(7.0)
    buf, view, r = _out((c.m, c.n), 2, 2)
    rkw = {k: v for k, v in kw.items() if k != "a2_off"}
    _C.gemm_halves3_nt_bn_reduce(a, b, sa, sb, piece_b, c.K, st2, o.a2_off, out=view, **rkw)
    _last(HC.expected_nt(c.K, 0, int(c.frag), "reduce"))
    assert torch.equal(st2.part, st.part) and torch.equal(st2.pmax, st.pmax)
    assert bool((buf.view(torch.int32) == SC.SENTINEL32).all()), "the reduce-only launch stored something"
    xi = _up(rng.integers(-3, 4, size=(c.m, c.n)).astype(F32))
    st3 = _C.BnBwdStats(xi, torch.zeros(c.n, device=DEV), torch.ones(c.n, device=DEV), None, None, False, 0.0, 1)
    for (pad, off) in ((2, 2), (2 if c.n % 4 == 2 else 0, 0)):          # float2 and (n + pad a multiple of 4) float4 stores of dx
        buf, view, r = _out((c.m, c.n), pad, off)
        _C.gemm_halves3_nt_bn_apply(a, b, sa, sb, piece_b, c.K, st3, o.a2_off, None, None, float(c.m), out=view, **rkw)
        _last(HC.expected_nt(c.K, 0, int(c.frag), "apply"))
        _check("nt", (c.tag, c.seed, "bnapply", pad), view.cpu().numpy(), s, True)
        assert SC.guards_intact(buf, view, r)


# ------------------------------------------------------------------------------------------------ NT, grouped
def _run_ng(o):
    c = o.c
    a, b = _rows(o.afull, c.m), _rows(o.bfull, c.b_rows)
    buf, view, r = _out((c.m, c.width), c.pad, c.off)
    slots = torch.zeros(int(_C._lib.bot_absmax_slots()), dtype=torch.int32, device=DEV) if c.absmax else None
    tiles = (c.m + 255) // 256
    stats = None
    if c.stats:
        stats = tuple(torch.full(sh, float("nan"), device=DEV) for sh in ((tiles, 2, c.width), (tiles, 2, c.width), (tiles, c.width)))
        for t in stats:
            t.view(torch.int32).fill_(SC.SENTINEL32)
    _C.gemm_halves3_nt_grouped(a, b, _up(o.sa), _up(o.sb), c.a2_off, c.b2_off, view, [list(g) for g in c.groups], c.k_seg, mode=c.mode,
                               col_scale=None if o.cs is None else _up(o.cs), col_shift=None if o.ch is None else _up(o.ch), relu=c.relu, absmax=slots,
                               stats=stats)
    _last(HC.expected_nt_grouped(c.groups, c.k_seg, c.mode, c.stats))
    assert SC.guards_intact(buf, view, r), c
    return view.cpu(), slots, stats


@pytest.mark.parametrize("c", HC.ng_cases(), ids=_ids(HC.ng_cases()))
def test_nt_grouped(c):
    o = HC.make_ng(c)
    r = HC.ng_reference(o)
    exact = c.regime == "exact"
    if exact:
        HC.assert_exact("nt_grouped", o)
    view, slots, stats = _run_ng(o)
    got, w = view.numpy(), r["written"]
    assert bool((view.view(torch.int32).numpy()[~w] == SC.SENTINEL32).all()), "an output column outside every group was written"
    if exact:
        bad = ~HC.same_bits(got[w], r["val"][w].astype(F32))
        assert not bad.any(), (c.tag, int(bad.sum()), got[w][bad][:4], r["val"][w][bad][:4])
    else:
        err, bound = np.abs(got[w].astype(F64) - r["val"][w]), r["bound"][w]
        ratio = float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
        WORST["nt_grouped"] = max(WORST.get("nt_grouped", 0.0), ratio)
        print(f"nt_grouped {c.tag} {c.seed}: worst error / bound {ratio:.3f}")
        assert ratio <= 1.0, (c, ratio)
    if c.absmax:         # the largest |stored value| over the slot set (WHICH slot a wave publishes into depends on the grid)
        stored = np.abs(got[w])
        assert int(slots.max()) == int(HC.bits32(stored[~np.isnan(stored)].max()).reshape(-1)[0]), c
    if c.stats:
        part, minmax, pivot = (t.cpu() for t in stats)
        col = w[0]
        for t in (part[:, 0], part[:, 1], minmax[:, 0], minmax[:, 1], pivot):
            assert bool((t.view(torch.int32).numpy()[:, ~col] == SC.SENTINEL32).all()), "statistics of a column no group writes"
        st = HC.stored_stats(np.where(w, got, 0.0).astype(F32), w, c.m)
        assert HC.same_bits(pivot.numpy()[:, col], st["pivot"][:, col].astype(F32)).all()
        assert HC.same_bits(minmax[:, 0].numpy()[:, col], st["min"][:, col].astype(F32)).all()
        assert HC.same_bits(minmax[:, 1].numpy()[:, col], st["max"][:, col].astype(F32)).all()
        for k, e, t in (("sum", "e_sum", part[:, 0]), ("sumsq", "e_sumsq", part[:, 1])):
            err = np.abs(t.numpy()[:, col].astype(F64) - st[k][:, col])
            assert bool((err <= st[e][:, col]).all()), (c.tag, k, float((err / np.maximum(st[e][:, col], 1e-300)).max()))
    RAN.add("nt_grouped")


# ------------------------------------------------------------------------------------------------ TN
def _run_tn(o):
    c = o.c
    x, d = _rows(o.xfull, c.n), _rows(o.dfull, c.n)
    buf, view, r = _out((c.K, c.P), c.ldo_pad, 0)
    floats = int(_C._lib.bot_gemm_halves3_tn_workspace_floats(c.n, o.kp, o.pp))
    s, launched, rps = HC.tn_splits(c.n, o.kp, o.pp)
    assert floats == s * o.kp * o.pp, (floats, s)
    ws = torch.full((floats + 64,), float("nan"), device=DEV)
    ws[floats:].view(torch.int32).fill_(SC.SENTINEL32)
    sx, sd, sd2 = _up(o.sx), _up(o.sd), (_up(o.sd2) if c.p_split else None)
    rc = _C._lib.bot_gemm_halves3_tn2_f32(c.n, c.K, c.P, o.kp, o.pp, sx.data_ptr(), sd.data_ptr(), _C._ptr(sd2), c.p_split, x.data_ptr(), o.ldx, o.x2_off, d.data_ptr(),
                                          o.ldd, o.d2_off, view.data_ptr(), c.P + c.ldo_pad, ws.data_ptr(), 0, _C._stream())
    _C._check(rc, "gemm_halves3_tn2")
    _last(HC.expected_tn())
    assert SC.guards_intact(buf, view, r), c
    assert bool((ws[floats:].view(torch.int32) == SC.SENTINEL32).all()), "wrote past the workspace"
    return view.cpu().numpy(), launched


@pytest.mark.parametrize("c", HC.tn_cases(), ids=_ids(HC.tn_cases()))
def test_tn(c):
    o = HC.make_tn(c)
    s = HC.tn_reference(o)
    got, launched = _run_tn(o)
    _check("tn", (c.tag, c.seed), got, s, c.regime == "exact", splits=launched)
    RAN.add("tn")


# ------------------------------------------------------------------------------------------------ TN, grouped
def _run_tg(o):
    c = o.c
    x, d = _rows(o.xfull, c.n), _rows(o.dfull, c.n)
    buf = torch.empty(SC.GUARD + c.out_floats + SC.GUARD, dtype=torch.float32, device=DEV)
    buf.view(torch.int32).fill_(SC.SENTINEL32)
    out = buf[SC.GUARD:SC.GUARD + c.out_floats]
    floats = int(_C._lib.bot_gemm_halves3_tn_grouped_workspace_floats(c.n, len(c.tiles)))
    assert floats == HC.tn_grouped_splits(c.n, len(c.tiles))[0] * len(c.tiles) * 192 * 192
    _C.gemm_halves3_tn_grouped(x, d, _up(o.sx), _up(o.sd), c.x2_off, c.d2_off, out, [list(t) for t in c.tiles])
    _last(HC.expected_tn_grouped(c.tiles))
    return buf.cpu()


@pytest.mark.parametrize("c", HC.tg_cases(), ids=_ids(HC.tg_cases()))
def test_tn_grouped(c):
    o = HC.make_tg(c)
    val, s, w = HC.tg_reference(o)
    if c.regime == "exact":
        HC.assert_exact("tn_grouped", o)
    buf = _run_tg(o)
    got = buf[SC.GUARD:SC.GUARD + c.out_floats].numpy()
    keep = np.ones(buf.numel(), bool)
    keep[SC.GUARD:SC.GUARD + c.out_floats] = ~w
    assert bool((buf.view(torch.int32).numpy()[keep] == SC.SENTINEL32).all()), "wrote outside the tiles' valid blocks"
    _check("tn_grouped", (c.tag, c.seed), got[w], HC.Sum3(val[w], s.ab[w], s.nz[w]), c.regime == "exact", splits=HC.tn_grouped_splits(c.n, len(c.tiles))[1])
    RAN.add("tn_grouped")


# ------------------------------------------------------------------------------------------------ never read into a stored value
@pytest.mark.parametrize("entry", ("nt", "nt_frag", "nt_grouped", "tn", "tn_grouped"))
def test_nothing_outside_the_contract_reaches_a_stored_value(entry):
    """Exact cases of one entry point, once with zeros and once with NaN in every fp16 element outside the contract's index set (A and B
    rows past m and n, B rows of other groups, the duplicate piece, the tail rows of a fragment-major tile, x and d columns outside a tile's
    valid range, guard rows): the same bits.  The zero padding the contract DOES read (pieces padded to 64) stays zero in both."""
    if entry in ("nt", "nt_frag"):
        cs = [c for c in HC.nt_cases() if c.regime == "exact" and c.frag == (entry == "nt_frag") and c.tag in ("n", "frag", "b2_off>K", "K")][:4]
        run = lambda c, outside: (lambda o: _run_nt(o, _nt_operands(o), 0, c.pad, c.off))(HC.make_nt(c, outside))
    elif entry == "nt_grouped":
        cs = [c for c in HC.ng_cases() if c.regime == "exact"][:3]
        run = lambda c, outside: _run_ng(HC.make_ng(c, outside))[0].numpy()
    elif entry == "tn":
        cs = [c for c in HC.tn_cases() if c.regime == "exact" and c.tag == "widths"][:3]
        run = lambda c, outside: _run_tn(HC.make_tn(c, outside))[0]
    else:
        cs = [c for c in HC.tg_cases() if c.regime == "exact"][:3]
        run = lambda c, outside: _run_tg(HC.make_tg(c, outside)).numpy()
    assert len(cs) >= 3
    for c in cs:
        zero, nan = run(c, F16(0)), run(c, HC.NAN16)
        assert HC.same_bits(zero, nan).all(), (entry, c)
        assert entry in ("nt_grouped", "tn_grouped") or not np.isnan(nan).any()         # (the grouped outputs keep their sentinel between the blocks)


# ------------------------------------------------------------------------------------------------ data edges
def _same_poison(got, ref):
    """exactly the entries the float64 restatement poisons are non-finite (an infinite one with its sign), every other one bit for bit"""
    fin = np.isfinite(ref)
    assert np.array_equal(np.isfinite(got), fin), (np.argwhere(np.isfinite(got) != fin)[:5].tolist())
    assert np.array_equal(np.isnan(got), np.isnan(ref)) and np.array_equal(got[np.isinf(ref)], ref[np.isinf(ref)].astype(F32))
    assert HC.same_bits(got[fin], ref[fin].astype(F32)).all()
    return int((~fin).sum())


@pytest.mark.parametrize("frag", (False, True))
def test_nt_non_finite_and_zero_operands(frag):
    c = HC.NT(m=70, n=40, K=128, frag=frag, seed=901)
    o = HC.make_nt(c)
    a1, a2, b1, b2 = HC.nt_pieces(o)
    o.A[5, 17], o.A[33, o.a2_off + 100], o.A[60, 3] = np.inf, np.nan, -np.inf
    b1, b2 = b1.copy(), b2.copy()
    b2[7, 64], b1[21, 0] = np.inf, np.nan
    if frag:
        o.B = HC.frag_pack(b1, b2, HC.NAN16)
    else:
        o.B[:, :c.K], o.B[:, o.b2_off:o.b2_off + c.K] = b1, b2
    ref = HC.nt_reference(o, want_bound=False).val
    poisoned = _same_poison(_run_nt(o, _nt_operands(o), 0, 0, 0), ref)
    assert poisoned == 3 * c.n + 2 * c.m - 6             # three rows and two columns, no entry more
    # all-zero operands: +0 everywhere
    z = HC.make_nt(c)
    z.A[...] = 0
    if frag:
        z.B = np.zeros_like(z.B)
    else:
        z.B[...] = 0
    got = _run_nt(z, _nt_operands(z), 0, 0, 0)
    assert bool((got.view(np.int32) == 0).all())


def test_tn_non_finite_and_zero_operands():
    c = HC.TN(n=70, K=65, P=63, seed=902)
    o = HC.make_tn(c)
    o.X[11, 7], o.X[50, o.x2_off + 64], o.D[3, 20], o.D[69, o.d2_off + 62] = np.inf, np.nan, -np.inf, np.nan
    ref = HC.tn_reference(o, want_bound=False).val
    assert _same_poison(_run_tn(o)[0], ref) == 2 * c.P + 2 * c.K - 4
    z = HC.make_tn(c)
    z.X[...], z.D[...] = 0, 0
    assert bool((_run_tn(z)[0].view(np.int32) == 0).all())


# ------------------------------------------------------------------------------------------------ encoders
def _place16(rows, ld, lead):
    """an fp16 output of `rows` rows of pitch ld, `lead` halves behind a 16-byte aligned address, every word SENTINEL16 -> (buffer, view, numpy copy)"""
    n = 64 + lead + rows * ld + 64
    buf = torch.full((n,), SC.SENTINEL16, dtype=torch.int16, device=DEV).view(torch.float16)
    view = torch.as_strided(buf, (rows, ld), (ld, 1), 64 + lead)
    host = np.full(n, SC.SENTINEL16, dtype=np.int16).view(F16)
    return buf, view, host, host[64 + lead:64 + lead + rows * ld].reshape(rows, ld)


def _equal16(buf, host, tag):
    got = buf.cpu().numpy()
    bad = ~HC.same_bits(got, host)
    assert not bad.any(), (tag, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], host[bad][:4])


@pytest.mark.parametrize("n,F,pad,off,e", HC.encoder_cases())
def test_encoders_bit_for_bit(n, F, pad, off, e):
    rng = np.random.default_rng(100 * n + F)
    x = HC.edge_values(rng, (n, F), big=e is None)
    if e is None and x.size > 20:
        x.reshape(-1)[rng.integers(0, x.size)] = np.nan           # dropped by the maximum
    xbuf, xv = SC.place(torch.from_numpy(x), SC.Recipe(off=off, pad=pad), DEV)
    sc = HC.scale_of(HC.absmax_of(x))
    got_sc = _C.halves_scale(xv).cpu().numpy()
    assert HC.same_bits(got_sc, sc).all(), (got_sc, sc)
    if e is not None:
        sc = HC.pow2(e)
    dsc = _up(sc)
    piece = HC.piece_of(F)
    for order in (0, 1, 2):
        ld = (2 if order == 2 else 3) * piece + 2 * (order % 2)
        buf, view, host, hv = _place16(n, ld, 2 * order)
        _C._check(_C._lib.bot_halves_split_f16(xv.data_ptr(), xv.stride(0) if n > 1 else F + pad, n, F, dsc.data_ptr(), order, view.data_ptr(), ld, piece,
                                               _C._stream()), "halves_split")
        HC.split_expected(x, sc[0], order, piece, hv)
        _equal16(buf, host, ("split", n, F, order))
    got = _C.halves_split_frag(xv, dsc, piece).cpu().numpy().reshape(-1)
    assert HC.same_bits(got, HC.frag_expected(x, sc[0], piece)).all(), ("frag", n, F)
    # the format's promise: (h1 + h2) / s reproduces a finite x to 2^-22 of the largest entry (under halves_scale's own scale)
    if e is None:
        h1, h2s, _, _ = HC.encode(np.nan_to_num(x), sc[0])
        dec = (h1.astype(F64) + h2s.astype(F64) / HC.SHIFT) / float(sc[0])
        assert float(np.abs(dec - np.nan_to_num(x).astype(F64)).max()) <= 2.0 ** -22 * HC.absmax_of(x)


def test_encoders_column_ranges_heads_tail_slots_and_combine():
    rng = np.random.default_rng(9)
    dsc = _up(HC.pow2(4))
    # split_cols: an odd F inside an even width, in the last 256-column block too; every order; the rest of the buffer untouched
    for (n, F, width, col, piece, order, off) in ((17, 7, 10, 20, 128, 0, 0), (17, 9, 10, 118, 128, 1, 1), (5, 255, 256, 0, 320, 2, 2), (16, 257, 258, 62, 320, 0, 1),
                                                 (3, 1, 2, 318, 320, 2, 0), (4099, 33, 34, 30, 64, 1, 2)):
        x = HC.edge_values(rng, (n, F))
        xbuf, xv = SC.place(torch.from_numpy(x), SC.Recipe(off=off, pad=off), DEV)
        ld = (2 if order == 2 else 3) * piece + 4
        buf, view, host, hv = _place16(n, ld, 0)
        _C.halves_split_cols(xv, dsc, order, view, piece, col, width)
        HC.split_expected(x, 16.0, order, piece, hv, width=width, col=col)
        _equal16(buf, host, ("split_cols", n, F, width, col, order))
    # split_heads with and without padding columns, 8-byte aligned and odd rows
    for (n, H, D, DP, off, pad) in ((17, 3, 5, 8, 0, 0), (16, 2, 6, 6, 2, 0), (4099, 3, 250, 256, 0, 2), (15, 4, 1, 2, 1, 1)):
        x = HC.edge_values(rng, (n, H * D))
        xbuf, xv = SC.place(torch.from_numpy(x), SC.Recipe(off=off, pad=pad), DEV)
        h2_off = H * DP + 2
        buf, view, host, hv = _place16(n, 2 * h2_off, 2)
        _C._check(_C._lib.bot_halves_split_heads_f16(xv.data_ptr(), xv.stride(0), n, H, D, dsc.data_ptr(), view.data_ptr(), 2 * h2_off, h2_off, DP, _C._stream()),
                  "halves_split_heads")
        HC.heads_expected(x, 16.0, H, D, DP, h2_off, hv)
        _equal16(buf, host, ("split_heads", n, H, D, DP))
    # halves_tail: sources of other pitches, a zeroed segment
    n = 257
    s1, s2 = HC.edge_values(rng, (n, 3)), HC.edge_values(rng, (n, 6))
    b1, v1 = SC.place(torch.from_numpy(s1), SC.Recipe(off=1, pad=2), DEV)
    b2, v2 = SC.place(torch.from_numpy(s2), SC.Recipe(), DEV)
    buf, view, host, hv = _place16(n, 80, 0)
    _C.halves_tail([(4, 3, v1), (7, 5, None), (20, 6, v2)], dsc, view, 40)
    HC.tail_expected([(4, 3, s1), (7, 5, None), (20, 6, s2)], 16.0, 40, hv)
    _equal16(buf, host, "tail")
    # scales from the by-product slots: every maximum of the clamps' neighbourhood
    for m in (0.0, 1e-30, 2.0 ** -149, 1.0, 1.0 + 2.0 ** -23, 16384.0, 3e38, float("inf")):
        slots = torch.zeros(int(_C._lib.bot_absmax_slots()), dtype=torch.int32, device=DEV)
        slots[5] = int(HC.bits32(m).reshape(-1)[0])
        slots[40] = int(HC.bits32(m * 0.5).reshape(-1)[0]) if np.isfinite(m) else 0
        assert HC.same_bits(_C.halves_scale_from_slots(slots).cpu().numpy(), HC.scale_of(m)).all(), m
        if np.isfinite(m):
            with np.errstate(all="ignore"):
                want = HC.scale_of(float(F32(m) * F32(3.0)))
            want = np.array([min(want[0], F32(8.0) * F32(0.5))], F32)
            got = _C.halves_scale_from_slots(slots, mult=3.0, cap=_up(np.array([8.0, 0.125], F32)), cap_ratio=0.5).cpu().numpy()
            assert got[0] == want[0] and got[1] == F32(1.0) / want[0], (m, got, want)
    # tn_combine: small integers bit for bit, normal values under gamma(chunks + 3)
    for exact in (True, False):
        for (S, K, PP, P, rem) in ((1, 5, 8, 7, False), (5, 33, 64, 63, True), (8, 3, 4, 1, False)):
            gen = (lambda sh: rng.integers(-8, 9, size=sh).astype(F32)) if exact else (lambda sh: rng.standard_normal(sh).astype(F32))
            a, b = gen((S, K, 2 * PP)), gen((S, K, PP))
            ra, rb = (gen((K, 2 * PP)), gen((K, PP))) if rem else (None, None)
            got = _C.halves_tn_combine(_up(a), _up(b), P, None if ra is None else _up(ra), None if rb is None else _up(rb)).cpu().numpy()
            val, ab, terms = HC.tn_combine_reference(a, b, P, ra, rb)
            if exact:
                assert HC.same_bits(got, val.astype(F32)).all()
            else:
                assert bool((np.abs(got.astype(F64) - val) <= HC.gamma(terms + 3) * ab).all())


def test_second_half_where_s_x_leaves_float32_range():
    """Directed (it failed before csrc/halves.hip formed the second half with ONE fused multiply-add): where s x overflows float32 the
    second half is the infinity opposite to h1 - fp32(s x) - h1 = inf - inf was NaN - and where it underflows to zero it keeps the
    sign of x; in all five encoders alike."""
    x = np.array([[3e38, -3e38, -3e-42, 3e-42, 1.0, -0.0, 2.0 ** -126, -1e-40]], F32)
    for e, col, h1w, h2w in ((60, 0, np.inf, -np.inf), (60, 1, -np.inf, np.inf), (-20, 2, -0.0, -0.0), (-20, 3, 0.0, 0.0), (-30, 7, -0.0, -0.0)):
        h1, h2s, h2, _ = HC.encode(x, 2.0 ** e)
        for h, want in ((h1, h1w), (h2s, h2w), (h2, h2w)):
            assert HC.same_bits(h[0, col:col + 1], np.array([want], F16)).all(), (e, col, h[0, col], want)
        dsc, xd = _up(HC.pow2(e)), _up(x)
        for order in (0, 1, 2):
            buf, view, host, hv = _place16(1, 3 * 64, 0)
            _C.halves_split(xd, dsc, order, 64, out=view)
            HC.split_expected(x, 2.0 ** e, order, 64, hv)
            _equal16(buf, host, ("split", e, order))
        assert HC.same_bits(_C.halves_split_frag(xd, dsc, 64).cpu().numpy().reshape(-1), HC.frag_expected(x, 2.0 ** e, 64)).all()
        buf, view, host, hv = _place16(1, 32, 0)
        _C.halves_split_heads(xd, dsc, 2, 4, 6, out=view[:, :24])
        HC.heads_expected(x, 2.0 ** e, 2, 4, 6, 12, hv)
        _equal16(buf, host, ("heads", e))
        buf, view, host, hv = _place16(1, 32, 0)
        _C.halves_tail([(2, 8, xd)], dsc, view, 16)
        HC.tail_expected([(2, 8, x)], 2.0 ** e, 16, hv)
        _equal16(buf, host, ("tail", e))


# ------------------------------------------------------------------------------------------------ routes
def _halves_ops(a, b):
    """the NTOps of two gemm.Halves (left, right) for nt_reference"""
    o = HC.NTOps()
    o.c = HC.NT(m=a.n, n=b.n, K=a.piece, frag=b.order == 3, regime="seeded")
    o.A, o.a2_off, o.b2_off = a.buf.cpu().numpy(), a.h2_off, b.piece
    o.B = b.buf.cpu().numpy().reshape(-1) if b.order == 3 else b.buf.cpu().numpy()
    o.sa, o.sb, o.sa2 = a.scale.cpu().numpy(), b.scale.cpu().numpy(), None
    return o


def test_routes_at_their_thresholds(monkeypatch):
    """gemm.split / split_right / mm_nt / tn at NT_MIN_COLS (P = 191 / 192), NODUP_MIN_PIECE (piece 192 / 256), TN_MIN_OUT, N = 8191 / 8192
    and a tile grid of 16 / 17: the kernel that ran is the one the restated route names (or none of the family: the library), the value is
    the restatement's from the operand buffers the route was given."""
    monkeypatch.setattr(gemm, "FORCE", True)
    gen = torch.Generator(device=DEV).manual_seed(3)
    kw = dict(nodup=gemm.LEFT_NODUP, min_piece=gemm.NODUP_MIN_PIECE)
    for (m, K, P) in ((300, 150, 191), (300, 150, 192), (300, 192, 40), (300, 193, 40), (300, 256, 40)):
        x, w = torch.randn(m, K, device=DEV, generator=gen), torch.randn(P, K, device=DEV, generator=gen) * 0.1
        a, b = gemm.split(x, 0), gemm.split_right(w)
        assert a.order == HC.left_order(HC.piece_of(K), **kw) and b.order == HC.split_right_order(P, K, gemm.RIGHT_FRAG, gemm.NT_MIN_COLS, **kw), (m, K, P)
        got = gemm.mm_nt(a, b)
        want = HC.mm_nt_route(a.order, b.order, P, a.piece, gemm.NT_MIN_COLS)
        name = _C._lib.bot_last_kernel().decode()
        assert (name == want) if want != "lib" else (name not in HC.all_forms()), (m, K, P, name, want)
        _check("routes", ("mm_nt", m, K, P, want), got.cpu().numpy(), HC.nt_reference(_halves_ops(a, b)), False)
    for (N, K, P) in ((8192, 512, 1024), (8192, 512, 960), (8191, 512, 960), (8192, 3072, 128), (8192, 3073, 128)):
        x = torch.randn(N, K, device=DEV, generator=gen) * (torch.rand(N, 1, device=DEV, generator=gen) < 0.05)
        d = torch.randn(N, P, device=DEV, generator=gen) * 0.01
        a, b = gemm.split(x, 0), gemm.split(d, 0)
        got = gemm.tn(a, b)
        want = HC.tn_route(N, K, P, gemm.TN_MIN_OUT, gemm.TN_NARROW)
        name = _C._lib.bot_last_kernel().decode()
        assert (name == want) if want != "lib" else (name not in HC.all_forms()), (N, K, P, name, want)
        o = HC.NTOps()
        o.c = HC.TN(n=N, K=K, P=P, regime="seeded")
        o.X, o.D, o.x2_off, o.d2_off = a.buf.cpu().numpy(), b.buf.cpu().numpy(), a.h2_off, b.h2_off
        o.sx, o.sd, o.sd2 = a.scale.cpu().numpy(), b.scale.cpu().numpy(), None
        splits = 64 if want == "lib" else HC.tn_splits(N, a.piece, b.piece)[1] if want == HC.TN_FORMS["tn"] else HC.tn_grouped_splits(N, len(HC.tn_tiles(K, P)))[1]
        _check("routes", ("tn", N, K, P, want), got.cpu().numpy(), HC.tn_reference(o), False, splits=splits)


# ------------------------------------------------------------------------------------------------ the forms seen
def test_zz_every_form_was_reported():
    """after the four case lists: bot_last_kernel() has named every launch form (a partial run cannot know)"""
    if RAN != {"nt", "nt_grouped", "tn", "tn_grouped"}:
        pytest.skip("only a part of the case lists ran in this process")
    assert SEEN >= HC.all_forms() and {s for s in SEEN if s.startswith("bot::gemm_halves3")} == HC.all_forms(), sorted(HC.all_forms() - SEEN)
    print("worst error / bound per entry point:", {k: round(v, 4) for k, v in sorted(WORST.items())})
