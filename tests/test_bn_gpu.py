"""The BatchNorm + ReLU + dropout passes (csrc/dense.hip) on the MI355X against the float64 restatements of tests/bn_cases.py, at every
launch form the dispatch can produce (61 names, counted by the restatement; BC.cases() reaches each): after every call bot_last_kernel()
must be the name the restated dispatch expects; in the exact regime the forward, the gate, the sums, the column maxima, the apply pass
and both halves layouts equal float64 bit for bit; on seeded inputs every entry stays under the derived bounds (an entry whose
pre-activation lies within the forward's own rounding of zero may take either gate); the forward's zero pattern equals the restated
Philox mask at every form; every operand is a view into a guarded allocation whose guards, padding columns and (for the halves apply)
the columns between hD and hDP come back untouched; the by-products (absmax, bn_bwd_bound, hscale) bracket what they bound; every
reduction is bitwise reproducible; the second stages run on synthetic partials at every block-count boundary; data edges, non-finite
values, argument errors; and the directed ReLU gate test.  Called through the `_C` wrappers.

Measured on the MI355X (DESIGN §8 "BatchNorm passes"; run with -s to print them): all 61 launch forms named and launched, 209 chained
cases and 58 second-stage cases.  Largest error seen as a fraction of its derived bound: y 0.833, halves of y 0.643, sum_g 0.185,
sum_gx 0.211, max |g| 0.971, max |xhat| 0.978, dx 0.849, halves of dx 0.524, colstats mean 0.789, M2 0.212, colsum 0.263, invstd 0.222,
running mean / variance 0.349 / 0.315, wide second-stage sums 0.976, tiles mean 0.952, tiles invstd 0.343; the composed call y 0.385,
dx 0.142 (eval 0.317), dweight 0.084, dbias 0.070.  rsqrtf: 7.8697e-08 = 1.320 U at the argument 2.60770073e+17 (BC.RSQRT_MEASURED).
The directed gate test FAILED before the fix, as the float32 emulation predicted: dx != 0 differed from the forward's y > 0 at 1 809 of
5 160 entries and sum_g from the count of positive y in 40 of 40 columns; with every site on common.h bn_pre, 0 and 0, and 0 of 40
columns in the NT by-product.  `bn_vec` never returns 2 (BC.unreachable_vec2): the <2> instantiations are dead code, left in place."""
import math
import types

import numpy as np
import pytest
import torch

from bot_amd import _C
from tests import _oracle_backend as OB
from tests import bn_cases as BC
from tests import spmm_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = BC.U
WORST, SEEN, RAN = {}, set(), set()
TAGS = ("rows", "cols", "big", "place", "heads")


@pytest.fixture(autouse=True)
def _restore_switches():
    yield
    _C.SEED_OFFSET = None


def _d(t):
    return None if t is None else t.to(DEV)


def _last(want=None):
    name = _C._lib.bot_last_kernel().decode()
    SEEN.add(name)
    if want is not None:
        assert name == want, (name, want)
    return name


def _poison(n, cols, dtype):
    """The wrappers allocate the halves operand of the forward themselves: leave a sentinel in the block the allocator hands out next,
    so that a column the kernel never writes does not hold a previous call's (correct) bits."""
    t = torch.full((n, cols), SC.SENTINEL16 if dtype == torch.int16 else float("nan"), dtype=dtype, device=DEV)
    del t


def _bad(c, bad):
    assert not bad, (c, bad)


def _sync_seed(i):
    _C.SEED_OFFSET = None if i.off is None else torch.tensor([i.off], dtype=torch.int64, device=DEV)


def run_chain(c, k):
    i = BC.make_inputs(c, k)
    r = BC.reference(i)
    exact = c.regime == "exact"
    if exact:
        BC.assert_exact(i, r)
    else:
        assert BC.undecided_share(i, r) <= BC.UNDECIDED_SHARE
    names = BC.expected_names(c)
    n, F = c.n, c.F
    tag = c.regime
    _sync_seed(i)
    _, x = SC.place(i.x, c.rx, DEV)
    _, dy = SC.place(i.dy, c.rdy, DEV)
    assert x.data_ptr() % 16 == 4 * c.rx.off and dy.data_ptr() % 16 == 4 * c.rdy.off
    mean, invstd, w, b = _d(i.mean), _d(i.invstd), _d(i.w), _d(i.b)
    bad = []
    keep, sure = r["keep"], r["pre"].abs() > r["e_pre"]

    # ---- statistics
    s = BC.stats64(i.x, i.eps, i.momentum, i.rm, i.rv, 7)
    m_d, m2_d = _C.colstats(x)
    _last(names["partial"])
    pow2 = n & (n - 1) == 0
    BC.check_values(bad, WORST, "colstats mean", exact and pow2, m_d.cpu(), s["mean"], s["e_mean"])
    BC.check_values(bad, WORST, "colstats m2", exact and pow2, m2_d.cpu(), s["m2"], s["e_m2"])
    cs = _C.colsum(x)
    _last(names["partial"])
    BC.check_values(bad, WORST, "colsum", exact, cs.cpu(), s["sum"], s["e_sum"])
    assert torch.equal(cs, _C.colsum(x))
    rm, rv, nbt = _d(i.rm), _d(i.rv), torch.tensor([7], dtype=torch.int64, device=DEV)
    mu_d, is_d = _C.bn_stats(x, i.eps, i.momentum, rm, rv, nbt)
    _last(names["partial"])
    assert torch.equal(mu_d, m_d) and int(nbt) == s["nbt"]
    BC.check_values(bad, WORST, "bn_stats invstd", False, is_d.cpu(), s["invstd"], s["e_invstd"])
    BC.check_values(bad, WORST, "running_mean", False, rm.cpu(), s["rm"], s["e_rm"])
    BC.check_values(bad, WORST, "running_var", False, rv.cpu(), s["rv"], s["e_rv"])
    rm2, rv2 = _d(i.rm), _d(i.rv)
    mu_h, is_h, hs_h = _C.bn_stats_halves(x, i.eps, i.momentum, rm2, rv2, None, w, b, c.p)
    _last(names["partial"])
    assert torch.equal(mu_h, mu_d) and torch.equal(is_h, is_d) and torch.equal(rm2, rm) and torch.equal(rv2, rv), (c, "bn_stats_halves: not bn_stats's bits")
    sc = float(hs_h[0])
    assert math.frexp(sc)[0] == 0.5 and float(hs_h[1]) == 1.0 / sc, (c, sc)
    y_own = _C.bn_act_fwd(x, mu_d, is_d, w, b, c.relu, c.p, i.seed)           # the epilogue on the statistics the call itself formed
    top = float(y_own.abs().max())
    assert top * sc < 2.0 ** 15, (c, top, sc)
    b64, s64 = BC.bound64(i.x, mu_d.cpu(), is_d.cpu(), i.w, i.b, c.p)
    i_own = types.SimpleNamespace(**{**vars(i), "mean": mu_d.cpu(), "invstd": is_d.cpu()})
    top64 = float(BC.reference(i_own, want_dx=False)["y"].abs().max())
    if top64 * float(s64[0]) > 2.0 ** 6:           # what the restatement says the bound leaves: then the device's must as well
        assert top * sc > 2.0 ** 5, (c, top, sc)
    assert sc in (float(s64[0]), float(OB._pow2_scale(float(b64.max()) * (1 + 1e-5))[0]), float(OB._pow2_scale(float(b64.max()) * (1 - 1e-5))[0])), (c, sc, s64)

    # ---- forward
    ybuf, y = SC.place_out((n, F), c.ry, DEV)
    _C.bn_act_fwd(x, mean, invstd, w, b, c.relu, c.p, i.seed, out=y)
    _last(names["fwd"])
    assert SC.guards_intact(ybuf, y, c.ry), (c, "y guards")
    got_y = y.cpu()
    BC.check_values(bad, WORST, "fwd y " + tag, exact, got_y, r["y"], r["e_y"])
    want_nz = keep & (r["pre"] > 0) if c.relu else keep
    assert torch.equal((got_y != 0)[sure], want_nz[sure]), (c, "the zero pattern is not the restated mask")
    if "fwd_h3" in names:
        piece = BC.piece_of(F)
        hs = OB._pow2_scale(float(r["y"].abs().max()))
        hsd, s_ = _d(hs), float(hs[0])
        for kind, pieces, want_y in (("fwd_h3", 3, True), ("fwd_h2", 2, True), ("fwd_h_only", 2, False)):
            ybuf, y = SC.place_out((n, F), c.ry, DEV)
            _poison(n, pieces * piece, torch.int16)
            y2, buf = _C.bn_act_fwd(x, mean, invstd, w, b, c.relu, c.p, i.seed, halves=(hsd, piece, pieces), want_y=want_y, out=y if want_y else None)
            _last(names[kind])
            got_h = buf.view(torch.int16).cpu()
            if want_y:
                assert SC.guards_intact(ybuf, y, c.ry) and torch.equal(y.cpu().view(torch.int32), got_y.view(torch.int32)), (c, kind, "y differs from the plain forward")
            else:
                assert y2 is None
            pad = torch.ones(n, pieces * piece, dtype=torch.bool)
            for q in range(pieces):
                pad[:, q * piece:q * piece + F] = False
            assert bool((got_h[pad] == 0).all()), (c, kind, "zero padding of the pieces")
            if pieces == 3:
                assert torch.equal(got_h[:, :F], got_h[:, piece:piece + F]), (c, "the duplicate piece")
            if exact:
                if not BC.same_halves(got_h, BC.fwd_halves_expected(r["y"].float(), s_, F, piece, pieces)):
                    bad.append(kind + " halves bits")
            else:
                BC.check_values(bad, WORST, "fwd halves " + tag, False, BC.fwd_halves_decode(got_h, s_, F, piece, pieces), r["y"],
                                BC.halves_bound(r["y"], r["e_y"], s_))

    # ---- backward: reduce (+ maxima and their bound)
    res = _C.bn_act_bwd_reduce(dy, x, mean, invstd, w, b, c.relu, c.p, i.seed, want_max=c.max)
    _last(names["reduce"])
    sg, sgx = res[0], res[1]
    BC.check_values(bad, WORST, "sum_g " + tag, exact, sg.cpu(), r["sum_g"], r["e_sum_g"] + U * r["sum_g"].abs())
    BC.check_values(bad, WORST, "sum_gx " + tag, exact, sgx.cpu(), r["sum_gx"], r["e_sum_gx"] + U * r["sum_gx"].abs())
    if c.max:
        nblk = BC.nblk_of(n)
        pm = res[2][BC.kRowBlocks * 2 * F:BC.kRowBlocks * 2 * F + nblk * 2 * F].view(nblk, 2, F).max(0).values.cpu()
        BC.check_values(bad, WORST, "max |g|", exact, pm[0], r["gmax"], BC.gamma(1) * r["gmax_alt"], alt=r["gmax_alt"])
        BC.check_values(bad, WORST, "max |xhat|", exact, pm[1], r["xmax"], BC.gamma(2) * r["xmax"])
        slots = _C.absmax_slots(DEV)
        sgi, sgxi = (None, None) if c.evalmode else (_d(i.sum_g), _d(i.sum_gx))
        _C.bn_bwd_bound(res[2], n, sgi, sgxi, i.total_count, w, invstd, slots)
        _last(names["bound"])
        val = float(slots.view(torch.float32).max())
        lo, hi = BC.bwd_bound64(i, r, c.evalmode)
        dx_true = r["dx_eval"] if c.evalmode else r["dx"]
        dx_alt = r["dx_eval_alt"] if c.evalmode else r["dx_alt"]
        true_max = float(torch.minimum(dx_true.abs(), dx_alt.abs()).max())
        assert val >= true_max and val <= hi * (1.0001 + 16 * U), (c, "bn_bwd_bound", val, true_max, lo, hi)
    res2 = _C.bn_act_bwd_reduce(dy, x, mean, invstd, w, b, c.relu, c.p, i.seed, want_max=c.max)
    assert torch.equal(res2[0], sg) and torch.equal(res2[1], sgx), (c, "the reduce pass is not reproducible")

    # ---- backward: apply
    sgi, sgxi = (None, None) if c.evalmode else (_d(i.sum_g), _d(i.sum_gx))
    want, alt, e = (r["dx_eval"], r["dx_eval_alt"], r["e_dx_eval"]) if c.evalmode else (r["dx"], r["dx_alt"], r["e_dx"])
    dbuf, dx = SC.place_out((n, F), c.rdx, DEV)
    slots = _C.absmax_slots(DEV)
    _C.bn_act_bwd_apply(dy, x, mean, invstd, w, b, c.relu, c.p, i.seed, sgi, sgxi, i.total_count, out=dx, absmax=slots)
    _last(names["apply"])
    assert SC.guards_intact(dbuf, dx, c.rdx), (c, "dx guards")
    got_dx = dx.cpu()
    BC.check_values(bad, WORST, "dx " + tag, exact, got_dx, want, e, alt=alt)
    assert float(slots.view(torch.float32).max()) == float(got_dx.abs().max()), (c, "absmax is not max |dx| of what the call wrote")
    if c.hd:
        hD, hDP = c.hd
        ldh, col0, h2_off = BC.heads_layout(F, hD, hDP)
        hs = OB._pow2_scale(float(want.abs().max()))
        hsd, s_ = _d(hs), float(hs[0])
        mask = BC.heads_mask(n, F, hD, hDP)
        for kind, with_dx in (("apply_h", True), ("apply_h_only", False)):
            hbuf = torch.full((2 * SC.GUARD + n * ldh,), SC.SENTINEL16, dtype=torch.int16, device=DEV)
            hout = hbuf[SC.GUARD:SC.GUARD + n * ldh].view(n, ldh).view(torch.float16)
            dbuf, dx = SC.place_out((n, F), c.rdx, DEV)
            _C.bn_act_bwd_apply_halves(dy, x, mean, invstd, w, b, c.relu, c.p, i.seed, sgi, sgxi, i.total_count, hsd, hout[:, col0:], hD, hDP,
                                       out=dx if with_dx else None, h2_off=h2_off)
            _last(names[kind])
            if with_dx:
                assert SC.guards_intact(dbuf, dx, c.rdx) and torch.equal(dx.cpu().view(torch.int32), got_dx.view(torch.int32)), (c, kind, "dx differs from the plain apply")
            hb = hbuf.cpu()
            assert bool((hb[:SC.GUARD] == SC.SENTINEL16).all()) and bool((hb[SC.GUARD + n * ldh:] == SC.SENTINEL16).all()), (c, kind, "halves guards")
            got_h = hb[SC.GUARD:SC.GUARD + n * ldh].view(n, ldh)
            assert bool((got_h[~mask] == SC.SENTINEL16).all()), (c, kind, "a padding column between hD and hDP, or the gap, was written")
            if exact:
                if not BC.same_halves(got_h, BC.heads_expected(want.float(), s_, F, hD, hDP)):
                    bad.append(kind + " halves bits")
            else:
                assert bool((got_h[mask] != SC.SENTINEL16).all())
                BC.check_values(bad, WORST, "dx halves " + tag, False, BC.heads_decode(got_h, s_, F, hD, hDP), want,
                                BC.halves_bound(want, e, s_), alt=alt)
    _bad(c, bad)
    RAN.add(k)


@pytest.mark.parametrize("tag", TAGS)
def test_bn_chain_fp64(tag):
    """Every case of BC.cases() with this tag: statistics, forward (plain, halves at 3 and 2 pieces, halves only), reduce (+ maxima and
    bound), apply (+ halves), each against float64 with the launch form named."""
    for k, c in enumerate(BC.cases()):
        if c.tag == tag:
            run_chain(c, k)
    print({k: round(v, 3) for k, v in sorted(WORST.items())})


def test_bn_every_form_seen_fp64():
    """The names bot_last_kernel() reported are names of the enumeration, and after the whole case list they are all of them."""
    if len(RAN) < len(BC.cases()):          # (run on its own: the chain first)
        for k, c in enumerate(BC.cases()):
            if k not in RAN:
                run_chain(c, k)
    bn = {s for s in SEEN if any(t in s for t in ("bn_", "colstats_", "pair_final_wide"))}
    assert bn <= BC.all_forms(), sorted(bn - BC.all_forms())
    missing = BC.all_forms() - set(BC.SECOND_STAGES[1:]) - bn
    assert not missing, sorted(missing)
    print(len(bn), "launch forms seen;", len(RAN), "cases")


# ------------------------------------------------------------------------------------------------ the second stages on synthetic partials
@pytest.mark.parametrize("regime", ("exact", "seeded"))
def test_bn_wide_second_stages_fp64(regime):
    """pair_final_wide / bn_bwd_bound_wide / bn_bwd_finish_wide on partials the test fills: the sums against float64 (bit for bit on
    integer partials), the bound against its own formula in float64 from the same operands, two-sided."""
    rng = np.random.default_rng(5)
    for kind, nblk, F, _ in BC.stage_cases():
        if kind != "wide":
            continue
        n = 256 * nblk
        for batch in (True, False):
            w = BC._f(rng.normal(0, 1, F)) if batch else None
            invstd = BC._f(np.exp(rng.normal(0, 0.5, F)))
            st = _C.BnBwdStats(torch.empty(n, F, device=DEV), torch.zeros(F, device=DEV), _d(invstd), _d(w), None, True, 0.0, 1)
            if regime == "exact":
                part, pmax = BC._f(rng.integers(-8, 9, (nblk, 2, F))), BC._f(rng.integers(0, 9, (nblk, 2, F)))
            else:
                part, pmax = BC._f(rng.normal(0, 3, (nblk, 2, F))), BC._f(np.abs(rng.normal(0, 3, (nblk, 2, F))))
            pmax[nblk - 1, :, F - 1] = 50.0            # the largest column maximum sits in the last block, last column
            st.part.copy_(part), st.pmax.copy_(pmax)
            sg, sgx = st.sums()
            _last("bot::pair_final_wide_kernel")
            a, b_, ea, eb = BC.pair64(part)
            bad = []
            BC.check_values(bad, WORST, "wide sums", regime == "exact", sg.cpu(), a, ea)
            BC.check_values(bad, WORST, "wide sums", regime == "exact", sgx.cpu(), b_, eb)
            assert not bad, (nblk, F, bad)
            cinv = float(np.float32(1.0 / n))
            gm, xm = pmax[:, 0].max(0).values.double(), pmax[:, 1].max(0).values.double()
            t = gm + (sg.cpu().double().abs() * cinv + xm * sgx.cpu().double().abs() * cinv if batch else 0.0)
            form = float(((w.double().abs() if w is not None else 1.0) * invstd.double() * t).max()) * float(np.float32(1.0001))
            s1, s2, s3 = _C.absmax_slots(DEV), _C.absmax_slots(DEV), _C.absmax_slots(DEV)
            st.bound(sg if batch else None, sgx if batch else None, n, s1)
            _last("bot::bn_bwd_bound_wide_kernel")
            fg, fgx = st.finish(batch, n, s2)
            _last("bot::bn_bwd_finish_wide_kernel")
            st.finish(batch, n, s3)
            assert torch.equal(fg, sg) and torch.equal(fgx, sgx) and torch.equal(s1, s2) and torch.equal(s2, s3), (nblk, F, batch)
            val = float(s1.view(torch.float32).max())
            assert abs(val - form) <= 16 * U * form, (nblk, F, batch, val, form)
    print({k: round(v, 3) for k, v in sorted(WORST.items()) if k.startswith("wide")})


def _tiles_inputs(rng, nblk, F, last):
    n = 256 * (nblk - 1) + last
    X = rng.normal(0, 1, (n, F)) * np.exp(rng.normal(0, 0.5, F)) + rng.normal(0, 3, F)
    X = torch.from_numpy(X.astype(np.float32)).double()
    part, minmax, pivot = torch.empty(nblk, 2, F), torch.empty(nblk, 2, F), torch.empty(nblk, F)
    for bk in range(nblk):
        blk = X[256 * bk:min(256 * (bk + 1), n)]
        pivot[bk] = blk[0].float()
        d = blk - pivot[bk].double()
        part[bk, 0], part[bk, 1] = d.sum(0).float(), (d * d).sum(0).float()
        minmax[bk, 0], minmax[bk, 1] = blk.min(0).values.float(), blk.max(0).values.float()
    return n, X, part, minmax, pivot


def test_bn_tiles_second_stage_fp64():
    """colstats_tiles_final_kernel on per-block partials with per-block pivots, at every block-count boundary and last blocks of 1,
    255 and 256 rows: mean, invstd, the running statistics, the step counter and the scale from the bound, against float64 on the same
    partials."""
    rng = np.random.default_rng(9)
    for kind, nblk, F, last in BC.stage_cases():
        if kind != "tiles":
            continue
        n, X, part, minmax, pivot = _tiles_inputs(rng, nblk, F, last)
        w, b = BC._f(rng.normal(0, 1, F)), BC._f(rng.normal(0, 0.3, F))
        rm0, rv0 = BC._f(rng.integers(-2, 3, F)), BC._f(rng.integers(1, 4, F))
        outs = []
        for _ in range(2):
            rm, rv, nbt = _d(rm0), _d(rv0), torch.tensor([3], dtype=torch.int64, device=DEV)
            mu, inv, hs = _C.bn_stats_halves_partials(_d(part), _d(minmax), _d(pivot), n, 1e-5, 0.1, rm, rv, nbt, _d(w), _d(b), 0.5)
            _last("bot::colstats_tiles_final_kernel")
            outs.append((mu, inv, hs, rm, rv))
        assert all(torch.equal(p, q) for p, q in zip(*outs)) and int(nbt) == 4, (nblk, F, last, "not reproducible")
        r = BC.tiles_stats64(part, minmax, pivot, n)
        bad = []
        BC.check_values(bad, WORST, "tiles mean", False, mu.cpu(), r["mean"], r["e_mean"])
        BC.check_values(bad, WORST, "tiles invstd", False, inv.cpu(), r["invstd"], r["e_invstd"])
        den = max(n - 1, 1)
        m = float(np.float32(0.1))
        BC.check_values(bad, WORST, "tiles running_mean", False, rm.cpu(), rm0.double() * (1 - m) + m * r["mean"],
                        BC.gamma(4) * ((rm0.double() * (1 - m)).abs() + (m * r["mean"]).abs()) + m * r["e_mean"])
        BC.check_values(bad, WORST, "tiles running_var", False, rv.cpu(), rv0.double() * (1 - m) + m * r["m2"] / den,
                        BC.gamma(6) * ((rv0.double() * (1 - m)).abs() + m * r["m2"] / den) + m * r["e_m2"] / den)
        assert not bad, (nblk, F, last, bad)
        # against the data the partials came from: the mean of the rows themselves
        assert float((mu.cpu().double() - X.mean(0)).abs().max()) <= 1e-5 * float(X.abs().max()), (nblk, F, last)
        dev = torch.maximum((r["mx"] - mu.cpu().double()).abs(), (r["mn"] - mu.cpu().double()).abs()) * inv.cpu().double()
        bound = float(((w.double().abs() * dev + b.double().abs()) / 0.5).max())
        sc = float(hs[0])
        assert sc in {float(OB._pow2_scale(bound * f)[0]) for f in (1.0, 1 + 1e-5, 1 - 1e-5)}, (nblk, F, last, sc, bound)
    print({k: round(v, 3) for k, v in sorted(WORST.items()) if k.startswith("tiles")})


# ------------------------------------------------------------------------------------------------ the fast reciprocal square root
def test_rsqrt_error_measured_fp64():
    """rsqrtf through bot_bn_stats_f32: two-row columns (+a, -a) with a 12-bit a have mean 0 and M2 / n = a^2 exactly (a float32 number),
    eps = 0: invstd is rsqrtf(a^2) and nothing else.  More than 4 U is a finding; the bounds use twice BC.RSQRT_MEASURED."""
    rng = np.random.default_rng(3)
    a = (rng.integers(2048, 4096, 4096).astype(np.float64) * 2.0 ** rng.integers(-30, 18, 4096)).astype(np.float32)
    x = torch.from_numpy(np.stack([a, -a])).to(DEV)
    mean, invstd = _C.bn_stats(x, 0.0, 0.0)
    assert bool((mean == 0).all())
    want = 1.0 / torch.from_numpy(a.astype(np.float64))
    rel = ((invstd.cpu().double() - want) / want).abs()
    at = int(rel.argmax())
    print("rsqrtf: largest relative error %.4e = %.3f U at argument %.9g" % (float(rel[at]), float(rel[at]) / U, float(a[at]) ** 2))
    assert float(rel.max()) <= 4 * U, "rsqrtf is off by more than 4 U: a finding"
    assert float(rel.max()) <= BC.RSQRT_ERR


# ------------------------------------------------------------------------------------------------ data edges
def _stats_under_bounds(x32, eps=1e-5):
    s = BC.stats64(x32, eps, 0.1)
    xd = _d(x32)
    mean, m2 = _C.colstats(xd)
    mu, inv = _C.bn_stats(xd, eps, 0.1)
    bad = []
    BC.check_values(bad, WORST, "edge mean", False, mean.cpu(), s["mean"], s["e_mean"])
    BC.check_values(bad, WORST, "edge m2", False, m2.cpu(), s["m2"], s["e_m2"])
    BC.check_values(bad, WORST, "edge invstd", False, inv.cpu(), s["invstd"], s["e_invstd"])
    assert not bad, bad
    return mean.cpu(), m2.cpu(), inv.cpu()


def test_bn_stats_data_edges_fp64():
    """An outlier pivot, a constant column, a far mean, tiny and huge magnitudes, one row: the statistics stay under the pivot-aware
    bounds of the restatement."""
    rng = np.random.default_rng(21)
    x = BC._f(rng.normal(0, 1, (1000, 6)))
    far = x.clone()
    far[0] = 1e6                                                        # the pivot row is an outlier
    _stats_under_bounds(far)
    const = x.clone()
    const[:, 2] = 3.25
    mean, m2, inv = _stats_under_bounds(const)
    assert float(m2[2]) == 0.0 and float(mean[2]) == 3.25
    assert abs(float(inv[2]) * math.sqrt(float(np.float32(1e-5))) - 1) <= BC.RSQRT_ERR + 4 * U
    _stats_under_bounds(x + 1e4)
    _stats_under_bounds(x * 1e15)
    mean, m2, inv = _stats_under_bounds(x * BC._f(1e-20))
    _stats_under_bounds(x[:1])                                          # n = 1: M2 = 0, the unbiased divisor is 1
    rm, rv = torch.zeros(6, device=DEV), torch.ones(6, device=DEV)
    _C.bn_stats(_d(x[:1]), 1e-5, 0.5, rm, rv)
    assert torch.equal(rv.cpu(), torch.full((6,), 0.5)) and torch.equal(rm.cpu(), (x[0] * 0.5))


def _all_outputs(x, dy, mean, invstd, w, b, p, seed):
    y = _C.bn_act_fwd(x, mean, invstd, w, b, True, p, seed)
    sg, sgx = _C.bn_act_bwd_reduce(dy, x, mean, invstd, w, b, True, p, seed)
    dx = _C.bn_act_bwd_apply(dy, x, mean, invstd, w, b, True, p, seed, sg, sgx, x.shape[0])
    m, m2 = _C.colstats(x)
    return [t.cpu() for t in (y, sg.unsqueeze(0), sgx.unsqueeze(0), dx, m.unsqueeze(0), m2.unsqueeze(0), _C.colsum(dy).unsqueeze(0))]


def test_bn_nonfinite_stays_in_its_column_fp64():
    """A NaN and an Inf planted in one column of x, and separately of dy: every other column of every output is bit-identical to the run
    without it; all-zero dy gives zero sums and a zero dx."""
    rng = np.random.default_rng(2)
    for F in (6, 8, 5):
        n = 37
        x, dy = _d(BC._f(rng.normal(0, 1, (n, F)))), _d(BC._f(rng.normal(0, 1, (n, F))))
        mean, invstd = _C.bn_stats(x, 1e-5, 0.1)
        w, b = _d(BC._f(rng.normal(0, 1, F))), _d(BC._f(rng.normal(0, 1, F)))
        clean = _all_outputs(x, dy, mean, invstd, w, b, 0.5, 77)
        for which in ("x", "dy"):
            for bad_value in (float("nan"), float("inf")):
                x2, dy2 = x.clone(), dy.clone()
                (x2 if which == "x" else dy2)[11, 3] = bad_value
                dirty = _all_outputs(x2, dy2, mean, invstd, w, b, 0.5, 77)
                others = [j for j in range(F) if j != 3]
                for a_, b_ in zip(clean, dirty):
                    assert torch.equal(a_[:, others].view(torch.int32), b_[:, others].view(torch.int32)), (F, which, bad_value)
        zero = _all_outputs(x, torch.zeros_like(dy), mean, invstd, w, b, 0.5, 77)
        assert not bool(zero[1].any()) and not bool(zero[2].any()) and not bool(zero[3].any())


def test_bn_argument_errors_fp64():
    """ldx < F, p = 1 and n = 0 on the statistics are refused with BotKernelError before any launch."""
    x = torch.zeros(64, device=DEV)
    mean, invstd = torch.zeros(8, device=DEV), torch.ones(8, device=DEV)
    narrow = torch.as_strided(x, (4, 8), (6, 1))
    before = _C._lib.bot_last_kernel().decode()
    for call in (lambda: _C.colstats(narrow), lambda: _C.colsum(narrow), lambda: _C.bn_stats(narrow, 1e-5, 0.1),
                 lambda: _C.bn_act_fwd(narrow, mean, invstd, None, None, True, 0.0, 1),
                 lambda: _C.bn_act_bwd_reduce(narrow, narrow, mean, invstd, None, None, True, 0.0, 1),
                 lambda: _C.bn_act_bwd_apply(narrow, narrow, mean, invstd, None, None, True, 0.0, 1, None, None, 4),
                 lambda: _C.bn_act_fwd(x.view(8, 8), mean, invstd, None, None, True, 1.0, 1),
                 lambda: _C.bn_stats_halves(x.view(8, 8), 1e-5, 0.1, None, None, None, None, None, 1.0),
                 lambda: _C.bn_stats(x[:0].view(0, 8), 1e-5, 0.1), lambda: _C.colstats(x[:0].view(0, 8)), lambda: _C.colsum(x[:0].view(0, 8))):
        with pytest.raises(_C.BotKernelError):
            call()
        assert _C._lib.bot_last_kernel().decode() == before       # (the name is recorded right before a launch)


# ------------------------------------------------------------------------------------------------ the composed call
@pytest.mark.parametrize("training", (True, False))
def test_bn_relu_dropout_composition_fp64(training):
    """ops.bn_relu_dropout on a strided input (8 bytes into rows of pitch F + 4: the quad form) against float64 BatchNorm + ReLU + the
    restated mask, forward and all three gradients, under the composed bounds: the statistics' errors e_mean, e_invstd move pre by
    |w| (invstd e_mean + |x - mean| e_invstd) and xhat by invstd e_mean + |x - mean| e_invstd (first order, times 1.01), which widens the
    undecided band, y, the sums (sum_gx by sum |g| times xhat's) and dx (by |w| e_invstd |inner| + |w| invstd (E_sum_g + |xhat| E_sum_gx
    + d xhat |sum_gx|) / n, and the rounding of float32(1 / n) itself).  Eval mode: the running statistics are constants, invstd = rsqrt(var + eps) within RSQRT_ERR + 2 U."""
    from bot_amd import ops
    n, F, p = 1000, 750, 0.5
    c = BC.Case(n=n, F=F, rx=BC.Recipe(off=2, pad=4), rdy=BC.R0, rdx=BC.R0, ry=BC.R0, relu=True, affine="wb", p=p if training else 0.0, off=None,
                regime="seeded", max=False, evalmode=not training, hd=None, tag="composed")
    i = BC.make_inputs(c, 77)
    bn = torch.nn.BatchNorm1d(F).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(i.w), bn.bias.copy_(i.b), bn.running_mean.copy_(i.rm), bn.running_var.copy_(i.rv)
    bn.train(training)
    _, xv = SC.place(i.x, c.rx, DEV)
    x = xv.requires_grad_(True)
    y = ops.bn_relu_dropout(x, bn, relu=True, p=p, training=training)
    y.backward(_d(i.dy))
    eps = float(np.float32(bn.eps))
    if training:
        s = BC.stats64(i.x, bn.eps, bn.momentum, i.rm, i.rv, 0)
        mean, invstd, e_mean, e_is = s["mean"], s["invstd"], s["e_mean"], s["e_invstd"]
        i.seed, i.off = y.grad_fn.epi.seed, None
    else:
        mean = i.rm.double()
        invstd = 1.0 / torch.sqrt(i.rv.double() + eps)
        e_mean, e_is = torch.zeros(F, dtype=torch.float64), invstd * (BC.RSQRT_ERR + 2 * U)
    w_abs, d_abs = i.w.double().abs(), (i.x.double() - mean).abs()
    dxhat = 1.01 * (invstd * e_mean + d_abs * e_is)
    i.mean, i.invstd, i.pre_slack, i.cinv = mean, invstd, w_abs * dxhat, 1.0 / n
    i.sum_g = i.sum_gx = torch.zeros(F)
    r0 = BC.reference(i, want_dx=False)
    i.sum_g, i.sum_gx = r0["sum_g"], r0["sum_gx"]
    r = BC.reference(i)
    assert BC.undecided_share(i, r) <= BC.UNDECIDED_SHARE
    bad = []
    f = BC.drop_factor(c.p)
    BC.check_values(bad, WORST, "composed y", False, y.detach().cpu(), r["y"], r["e_y"] + f * i.pre_slack)
    E_sg = r["e_sum_g"] + U * r["sum_g"].abs()
    E_sgx = r["e_sum_gx"] + U * r["sum_gx"].abs() + (r["g"].abs() * dxhat).sum(0) * (1 + 8 * U)
    BC.check_values(bad, WORST, "composed dbias", False, bn.bias.grad.cpu(), r["sum_g"], E_sg)
    BC.check_values(bad, WORST, "composed dweight", False, bn.weight.grad.cpu(), r["sum_gx"], E_sgx)
    if training:
        e_dx = r["e_dx"] + 2 * U * r["wis"].abs() * (r["mg"].abs() + r["xmgx"].abs()) + w_abs * e_is * r["inner"].abs() * 1.01 + r["wis"].abs() * (E_sg + r["xhat"].abs() * E_sgx + dxhat * r["sum_gx"].abs()) / n * 1.01
        BC.check_values(bad, WORST, "composed dx", False, x.grad.cpu(), r["dx"], e_dx, alt=r["dx_alt"])
        bad2 = []
        BC.check_values(bad2, WORST, "composed running_mean", False, bn.running_mean.cpu(), s["rm"], s["e_rm"])
        BC.check_values(bad2, WORST, "composed running_var", False, bn.running_var.cpu(), s["rv"], s["e_rv"])
        bad += bad2
    else:
        BC.check_values(bad, WORST, "composed dx eval", False, x.grad.cpu(), r["dx_eval"], r["e_dx_eval"] + w_abs * e_is * r["g"].abs() * 1.01, alt=r["dx_eval_alt"])
        assert torch.equal(bn.running_mean.cpu(), i.rm) and torch.equal(bn.running_var.cpu(), i.rv)
    assert not bad, bad
    print({k: round(v, 3) for k, v in sorted(WORST.items()) if k.startswith("composed")})


# ------------------------------------------------------------------------------------------------ the ReLU gate, forward against backward
def test_bn_gate_forward_equals_backward_fp64():
    """The directed gate test: rows within 64 float32 ulps of the ReLU boundary of columns whose (invstd, w, b) make the two float32
    expressions fmaf(v - mu, invstd w, b) and fmaf((v - mu) invstd, w, b) disagree (BC.gate_inputs asserts on the CPU that at least 5 %
    of the rows do).  With p = 0 and dy = 1 on eval statistics dx != 0 must hold exactly where the forward's y > 0, sum_g must count the
    positive y of a column, and the NT product's by-product must as well."""
    x, mean, invstd, w, b, share = BC.gate_inputs()
    assert share >= 0.05
    xd, md, isd, wd, bd = _d(x), _d(mean), _d(invstd), _d(w), _d(b)
    n, F = x.shape
    y = _C.bn_act_fwd(xd, md, isd, wd, bd, True, 0.0, 1)
    fwd = torch.from_numpy(BC.gate_emulation(x, mean, invstd, w, b)[0])
    assert torch.equal((y > 0).cpu(), fwd), "the forward's gate is not the float32 expression the emulation evaluates"
    ones = torch.ones(n, F, device=DEV)
    dx = _C.bn_act_bwd_apply(ones, xd, md, isd, wd, bd, True, 0.0, 1, None, None, n)
    sg, _ = _C.bn_act_bwd_reduce(ones, xd, md, isd, wd, bd, True, 0.0, 1)
    diff_apply = int(((dx != 0) != (y > 0)).sum())
    diff_reduce = int((sg.cpu() != (y > 0).sum(0).float().cpu()).sum())
    print("gate: %d of %d entries differ between forward and apply; %d of %d columns in the reduce pass" % (diff_apply, n * F, diff_reduce, F))
    assert diff_apply == 0 and diff_reduce == 0, (diff_apply, diff_reduce)
    # the NT product's by-product at its smallest fitting shape: integer operands make dy integers, exact through the halves product, so
    # sum_g must be the sum of dy over the rows the forward kept, exactly
    from bot_amd import gemm
    rng = np.random.default_rng(4)
    K = 64
    d, wt = _d(BC._f(rng.integers(-2, 3, (n, K)))), _d(BC._f(rng.integers(-1, 2, (F, K))))
    ws = gemm.split(wt, 1)
    piece = ws.piece
    sc = _C.halves_scale(d)
    db = _C.halves_split(d, sc, 2, piece)
    st = _C.BnBwdStats(xd, md, isd, wd, bd, True, 0.0, 1)
    assert st.fits(n, F, piece)
    dy = _C.gemm_halves3_nt(db, ws.buf, sc, ws.scale, piece, piece, piece, bn=st, a2_off=piece, n=F)
    assert "bnb" in _C._lib.bot_last_kernel().decode()
    assert torch.equal(dy, d @ wt.t()) and int((dy != 0).sum()) > n * F // 2
    sg_nt, _ = st.sums()
    want = (dy * (y > 0)).sum(0)
    diff_nt = int((sg_nt != want).sum())
    print("gate: %d of %d columns differ in the NT by-product" % (diff_nt, F))
    assert diff_nt == 0, diff_nt
