"""The SpMM sweeps (csrc/spmm.hip) on the MI355X against the float64 restatements of tests/spmm_cases.py, at every instantiation the
dispatchers can produce (265 names; tests/spmm_cases.cases() reaches each through every entry point that can record it): after every
call bot_last_kernel() must be the name the restated dispatch expects; in the exact regime (integer x, y, addend, weights that are
multiples of 0.25 with both zeros) out, dot, the halves bits and absmax equal float64 bit for bit, for every wperm choice, with and
without addend, with the zero-skip on and off; on seeded normal inputs every entry stays under the derived bounds; every operand is a
view into a guarded allocation whose guards must come back untouched; the flat layout against the rows layout and offset views against
aligned ones; the absmax by-product of both spmm_dot paths; non-finite values; and empty work.  Called through the `_C` wrappers; the
outputs the wrappers allocate themselves (bot_spmm_bcast_f32's out, bot_spmm_dot_bcast_f32's dot) have no guards.

With the zero-skip on (the default) the restatement expects what include/bot_gnn.h states: dot = 0.f where the weight is exactly 0; "on
equals off" is `out`, the halves and absmax bit for bit and dot wherever the weight is not 0, and the switch-off run is held to the full
restatement.

Measured on the MI355X: 265 instantiations launched and named (681 cases).  Largest error seen as a fraction of its derived bound (run
with -s to print them; DESIGN §8 "SpMM sweeps"): bot_spmm_f32 out 0.613; bot_spmm_dot_f32 out 0.480, dot 0.609; bot_spmm_dot_halves_f16
decoded halves 0.438, dot 0.240; bot_spmm_bcast_f32 out 0.487; bot_spmm_bcast_halves_f16 decoded halves 0.450; bot_spmm_dot_bcast_f32 out
0.448, dot 0.549; offset views out 0.469, halves 0.391, dot 0.036.  Seeded results were bitwise equal across VEC 4 / 1 / 2 for `out` of
every entry tried and differed for the dot products (the lane that holds an element, and so the order of its dot product's additions,
depends on VEC)."""
import functools

import pytest
import torch

from bot_amd import _C, blocked
from tests import attn_cases as AC
from tests import spmm_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = {}
GROUPS = SC.groups()
WEIGHT_SKIPPERS = ("spmm", "spmm_dot", "spmm_dot_halves")


@pytest.fixture(autouse=True)
def _restore_switches():
    yield
    _C.spmm_set_zero_skip(1)
    _C.SPMM_LAYOUT = None


@functools.lru_cache(maxsize=None)
def _graphs():
    """name -> (CPU graph, device graph), both directions built once; none of them is dense enough for the blocked sweep."""
    out = {}
    for name, g in SC.graphs():
        g.create_formats_()
        gd = g.to(DEV)
        gd.create_formats_()
        assert blocked.plan_for(gd.csc, g.number_of_src_nodes(), 2, 16) is None and blocked.plan_for(gd.csr, g.number_of_dst_nodes(), 2, 16) is None
        out[name] = (g, gd)
    return out


def _d(t):
    return None if t is None else t.to(DEV)


def _same(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _last():
    return _C._lib.bot_last_kernel().decode()


def run(o, dd, layout=None):
    """One call of o.case.entry on direction dd with every float operand placed under the case's recipe.  Returns (result dict of CPU
    tensors for SC.check, kernel name).  Asserts the guards of every output the test owns."""
    c, r = o.case, o.case.recipe
    H, D, n_rows, nnz = c.H, c.D, dd.n_rows, dd.nnz
    w, wperm = _d(o.w), _d(o.wperm)
    got = {}
    _, x = SC.place(o.x, r, DEV, contiguous=c.entry == "spmm_dot_bcast")
    assert x.data_ptr() % 16 == 4 * r.off
    y = SC.place(o.y, r, DEV)[1] if o.y is not None else None
    if "dot" in c.entry and c.entry != "spmm_dot_bcast":
        dbuf = torch.full((2 * SC.GUARD + nnz * H,), SC.SENTINEL32, dtype=torch.int32, device=DEV).view(torch.float32)
        dot = dbuf[SC.GUARD:SC.GUARD + nnz * H].view(nnz, H)
    if "halves" in c.entry:
        ldh, hsh, h2_off, col0, piece = SC.halves_layout(c, n_rows)
        hbuf = torch.full((2 * SC.GUARD + n_rows * ldh,), SC.SENTINEL16, dtype=torch.int16, device=DEV)
        hout = hbuf[SC.GUARD:SC.GUARD + n_rows * ldh].view(n_rows, ldh).view(torch.float16)
        hscale = _d(o.hscale)
    if c.entry == "spmm":
        obuf, out = SC.place_out((n_rows, H, D), r, DEV)
        addend = SC.place(o.addend, r, DEV)[1] if o.addend is not None else None
        _C.SPMM_LAYOUT = layout or ("flat" if c.flat else "rows")
        try:
            _C.spmm(dd, x, w, wperm, out=out, addend=addend)
        finally:
            _C.SPMM_LAYOUT = None
    elif c.entry == "spmm_dot":
        obuf, out = SC.place_out((n_rows, H, D), r, DEV)
        slots = _C.absmax_slots(DEV)
        _C.spmm_dot(dd, x, w, wperm, y, out=out, dot=dot, absmax=slots)
    elif c.entry == "spmm_dot_halves":
        assert _C.spmm_dot_halves_fits(x, y, hout[:, col0:], hsh, h2_off)
        _C.spmm_dot_halves(dd, x, w, wperm, y, hscale, hout[:, col0:], hsh, h2_off, dot=dot)
    elif c.entry == "spmm_bcast":
        res = _C.spmm_bcast(dd, x, w, wperm, head_outer=c.head_outer)
    elif c.entry == "spmm_bcast_halves":
        _C.spmm_bcast_halves(dd, x, w, wperm, hscale, hout, col0, hsh, h2_off, piece)
    else:
        obuf, out = SC.place_out((n_rows, D), r, DEV)
        _, got["dot"] = _C.spmm_dot_bcast(dd, x, w, wperm, y, out=out)
    name = _last()
    if c.entry in ("spmm", "spmm_dot", "spmm_dot_bcast"):
        assert SC.guards_intact(obuf, out, r), (c, "out guards")
        got["out"] = out.cpu().reshape(n_rows, -1, D)
    if c.entry == "spmm_bcast":
        got["out"] = (res.permute(1, 0, 2) if c.head_outer else res).contiguous().cpu()
    if c.entry == "spmm_dot":
        got["absmax"] = float(slots.view(torch.float32).max())
    if "dot" in c.entry and c.entry != "spmm_dot_bcast":
        guards = torch.cat([dbuf[:SC.GUARD], dbuf[SC.GUARD + nnz * H:]]).view(torch.int32)
        assert bool((guards == SC.SENTINEL32).all()), (c, "dot guards")
        got["dot"] = dot
    if got.get("dot") is not None:
        got["dot"] = got["dot"].cpu()
    if "halves" in c.entry:
        assert bool((torch.cat([hbuf[:SC.GUARD], hbuf[SC.GUARD + n_rows * ldh:]]) == SC.SENTINEL16).all()), (c, "halves guards")
        got["halves"] = hout.view(torch.int16).cpu()
    return got, name


def _ops(case, *args):
    """SC.make_ops for a call with the process default, zero-skip on: the restatement then expects dot = 0.f where the weight is 0."""
    o = SC.make_ops(case, *args)
    o.skip = case.entry in ("spmm_dot", "spmm_dot_halves")
    return o


def _skip_on_equals_off(o, on, off):
    """include/bot_gnn.h bot_spmm_set_zero_skip: on finite data `out` (fp32, halves, absmax) is the same bit for bit either way, and so is
    dot wherever the weight is not exactly 0."""
    rest = all((on.get(k) is None and off.get(k) is None) or (on[k] == off[k] if k == "absmax" else _same(on[k], off[k])) for k in ("out", "halves", "absmax"))
    live = o.w != 0 if on.get("dot") is not None else None
    return rest and (live is None or _same(on["dot"][live], off["dot"][live]))


def _equal(a, b):
    return all((a.get(k) is None and b.get(k) is None) or (a[k] == b[k] if k == "absmax" else _same(a[k], b[k])) for k in ("out", "dot", "halves", "absmax"))


def _expected(c):
    return SC.expected_kernel(c.entry, c.H, c.D, SC.case_vec(c.entry, c.H, c.D, c.recipe), c.weighted, c.flat, c.hpiece)


# ------------------------------------------------------------------------------------------------ 1. dispatch
def test_every_instantiation_is_launched_and_named():
    """Every case on the smallest graph: the recorded kernel is the one the restated dispatch expects, the result is exact, and the union
    of the names is every instantiation the dispatchers can produce."""
    g, gd = _graphs()["sweep128"]
    seen, fails = set(), []
    for i, c in enumerate(SC.cases()):
        d, n_cols, own = SC.direction(g, c.entry)
        dd = SC.direction(gd, c.entry)[0]
        wperm, addend, seed = SC.variant(i, 0)
        o = _ops(c, d, n_cols, own, "exact", seed, wperm, addend and c.entry == "spmm")
        got, name = run(o, dd)
        assert name == c.kernel == _expected(c), (c, name)
        bad = SC.check(o, got, SC.reference(o), True)
        if bad:
            fails.append((c.kernel, c.H, c.D, tuple(c.recipe), c.hpiece, wperm, bad))
        seen.add(name)
    assert not fails, (len(fails), fails[:12])
    assert seen == set(SC.all_instantiations()) and len(seen) == 265


# ------------------------------------------------------------------------------------------------ 2. both regimes, every case
@pytest.mark.parametrize("entry,vec", sorted(GROUPS))
def test_cases_against_fp64(entry, vec):
    """The group's cases on their graphs: exact regime bit for bit (zero-skip on and off, and on equal to off), seeded regime under the
    bounds, the kernel name after every call, the guards after every call (run)."""
    graphs = _graphs()
    index = {c: i for i, c in enumerate(SC.cases())}
    fails = []
    for c in GROUPS[(entry, vec)]:
        i = index[c]
        for gi, gname in enumerate(SC.graphs_for(c, i)):
            g, gd = graphs[gname]
            d, n_cols, own = SC.direction(g, entry)
            dd = SC.direction(gd, entry)[0]
            wperm, addend, seed = SC.variant(i, gi)
            for regime in ("exact", "normal"):
                o = _ops(c, d, n_cols, own, regime, seed, wperm, addend and entry == "spmm")
                ref = SC.reference(o)
                got, name = run(o, dd)
                assert name == c.kernel, (c, gname, name)
                bad = SC.check(o, got, ref, regime == "exact", WORST)
                if bad:
                    fails.append((c.kernel, c.H, c.D, tuple(c.recipe), c.hpiece, gname, regime, wperm, addend, bad))
                if entry in WEIGHT_SKIPPERS and c.weighted and regime == "exact":
                    _C.spmm_set_zero_skip(0)
                    off, name = run(o, dd)
                    _C.spmm_set_zero_skip(1)
                    assert name == c.kernel and _skip_on_equals_off(o, got, off), (c, gname, "zero-skip on != off")
                    o.skip = False                          # every dot product is computed
                    bad = SC.check(o, off, SC.reference(o), True)
                    if bad:
                        fails.append((c.kernel, c.H, c.D, tuple(c.recipe), c.hpiece, gname, "zero-skip off", wperm, addend, bad))
    for f in fails[:8]:
        print("\nFAIL", f)
    assert not fails, (len(fails), fails[:12])


# ------------------------------------------------------------------------------------------------ 3. layouts
def test_flat_layout_equals_rows_layout():
    """include/bot_gnn.h bot_spmm_set_layout: both all-heads forward layouts give bitwise identical results, in both regimes."""
    graphs = _graphs()
    n = 0
    for i, c in enumerate(SC.cases()):
        if not c.flat:
            continue
        for gname in ("lanes32", "lanes300", "sweep8"):
            g, gd = graphs[gname]
            d, n_cols, own = SC.direction(g, "spmm")
            for regime in ("exact", "normal"):
                o = _ops(c, d, n_cols, own, regime, i, SC.WPERMS[i % 3], i % 2 == 0)
                flat, name = run(o, gd.csc, "flat")
                assert name == c.kernel
                rows, name = run(o, gd.csc, "rows")
                assert "rows_kernel" in name or "spmm_kernel" in name
                assert _equal(flat, rows), (c, gname, regime)
                n += 1
    assert n == 8 * 3 * 2


OFFSET_SHAPES = (("spmm", 1, 40), ("spmm", 3, 40), ("spmm", 2, 264), ("spmm_dot", 1, 72), ("spmm_dot", 3, 128), ("spmm_dot_halves", 4, 36),
                 ("spmm_bcast", 3, 100), ("spmm_bcast_halves", 2, 64), ("spmm_dot_bcast", 4, 68))


@pytest.mark.parametrize("entry,H,D", OFFSET_SHAPES)
def test_offset_views_against_aligned_views(entry, H, D):
    """A D divisible by 4 at base offsets of 0, 4 and 8 bytes (VEC 4, 1, 2): in the exact regime the three results are equal bit for bit;
    on seeded inputs each is held to the bound, and whether they were bitwise equal across VEC is REPORTED (it is not documented)."""
    g, gd = _graphs()["lanes32"]
    d, n_cols, own = SC.direction(g, entry)
    dd = SC.direction(gd, entry)[0]
    for regime in ("exact", "normal"):
        res = []
        for off, vec in ((0, 4), (1, 1), (2, 2)):
            r = SC.Recipe(off=off)
            hp = SC._halves_piece(D) if entry == "spmm_bcast_halves" else None
            c = SC.Case(entry, H, D, r, True, False, hp, True, SC.expected_kernel(entry, H, D, vec, hpiece=hp), False)
            assert SC.case_vec(entry, H, D, r) == vec
            o = _ops(c, d, n_cols, own, regime, 77, "random", entry == "spmm")
            got, name = run(o, dd)
            assert name == c.kernel and f"<{vec}," in name, (c, name)
            assert not SC.check(o, got, SC.reference(o), regime == "exact", WORST, tag=" (offset view)"), (c, regime)
            res.append(got)
        same = _equal(res[0], res[1]) and _equal(res[0], res[2])
        if regime == "exact":
            assert same, (entry, H, D)
        else:
            print(f"\n{entry} H={H} D={D}: seeded results bitwise equal across VEC 4 / 1 / 2: {same}")


# ------------------------------------------------------------------------------------------------ 4. absmax
@pytest.mark.parametrize("H,D", [(1, 40), (3, 40), (3, 250), (2, 10), (9, 7), (5, 300)])
def test_absmax_byproduct_of_both_paths(H, D):
    """The rows path (the kernel's by-product for short rows, the combine pass's for long ones) and the head-major path (a separate pass
    over the result) both deliver exactly max |out|: with the maximum in a long row, in a short row, and on a graph without long rows."""
    for gname in ("lanes32", "lanes300", "square17long"):
        g, gd = _graphs()[gname]
        d, dd = g.csr, gd.csr
        vec = SC.case_vec("spmm_dot", H, D, SC.Recipe())
        c = SC.Case("spmm_dot", H, D, SC.Recipe(), True, False, None, True, SC.expected_kernel("spmm_dot", H, D, vec), False)
        deg = AC.degrees(d)
        for regime, boost in (("exact", None), ("normal", None), ("normal", "short")):
            o = _ops(c, d, g.number_of_dst_nodes(), g.csr2csc, regime, 5, "eid")
            if boost:                                       # the largest value into a short row: the weight of its first edge
                r = int(((deg >= 1) & (deg <= d.chunk)).nonzero()[0])
                o.w[int(o.wperm[int(d.indptr[r])])] = 1e4
            ref = SC.reference(o)
            got, name = run(o, dd)
            assert name == c.kernel and ("rows" in name) == ((H, D) in ((3, 40), (3, 250)))
            own = float(got["out"].abs().max())
            assert got["absmax"] == own > 0, (gname, regime, boost, got["absmax"], own)
            assert not SC.check(o, got, ref, regime == "exact"), (gname, regime, boost)
            if boost and d.n_long:
                assert int(got["out"].abs().amax((1, 2)).argmax()) not in d.long_rows.tolist()


# ------------------------------------------------------------------------------------------------ 5. non-finite values
NONFINITE = (("spmm", 1, 40, False), ("spmm", 3, 40, False), ("spmm", 3, 250, False), ("spmm", 3, 250, True), ("spmm", 6, 300, False),
             ("spmm_dot", 1, 40, False), ("spmm_dot", 3, 40, False), ("spmm_dot", 3, 250, False), ("spmm_dot_halves", 2, 72, False))


@pytest.mark.parametrize("entry,H,D,flat", NONFINITE)
def test_nonfinite_values_stay_where_they_belong(entry, H, D, flat):
    """A NaN in ONE head slab of ONE source row reaches exactly that head of the rows (and the dot products of the edges) that gather
    it, every other entry keeps its bits; an Inf weight on an edge whose source slab is zero makes that head of that row NaN and nothing
    else.  Zero-skip off and on (the weights are non-zero, so both read every row)."""
    g, gd = _graphs()["lanes32"]
    d, n_cols, own = SC.direction(g, entry)
    dd = SC.direction(gd, entry)[0]
    r = SC.FLAT_RECIPES[0] if flat else SC.Recipe()
    vec = SC.case_vec(entry, H, D, r)
    c = SC.Case(entry, H, D, r, True, flat, None, True, SC.expected_kernel(entry, H, D, vec, True, flat), False)
    rows, src = AC.rows_of(d), d.indices.long()
    o = _ops(c, d, n_cols, own, "normal", 9, "random")
    o.w = o.w.abs() + 0.5
    o.hscale = torch.tensor([1.0, 1.0])
    perm = o.wperm.long()
    s, h = int(src[len(src) // 2]), H - 1
    k0 = int((AC.degrees(d)[rows] >= 3).nonzero()[0])        # an edge of a row with company
    for skip in (0, 1):
        _C.spmm_set_zero_skip(skip)
        base, name = run(o, dd)
        assert name == c.kernel
        base_out = base["out"] if "out" in base else SC.halves_decode(o, base["halves"])
        assert bool(torch.isfinite(base_out).all())
        # the NaN slab
        x = o.x.clone()
        o.x = x.clone()
        o.x[s, h] = float("nan")
        got, _ = run(o, dd)
        o.x = x
        out = got["out"] if "out" in got else SC.halves_decode(o, got["halves"])
        hit = torch.zeros(d.n_rows, H, dtype=torch.bool)
        hit[rows[src == s], h] = True
        assert hit.any() and bool((torch.isnan(out).all(2) == hit).all()) and bool((torch.isnan(out).any(2) == hit).all()), (c, skip)
        keep = ~hit[:, :, None].expand_as(out)
        assert torch.equal(out[keep], base_out[keep])
        if "dot" in got:
            dhit = torch.zeros(d.nnz, H, dtype=torch.bool)
            dhit[perm[src == s], h] = True
            assert bool((torch.isnan(got["dot"]) == dhit).all()) and torch.equal(got["dot"][~dhit], base["dot"][~dhit])
        # Inf times zero
        w = o.w.clone()
        o.w, o.x = w.clone(), x.clone()
        o.w[perm[k0], 0] = float("inf")
        o.x[src[k0], 0] = 0.0
        got, _ = run(o, dd)
        o.w[perm[k0], 0] = 1.0
        fin, _ = run(o, dd)
        o.w, o.x = w, x
        out = got["out"] if "out" in got else SC.halves_decode(o, got["halves"])
        fout = fin["out"] if "out" in fin else SC.halves_decode(o, fin["halves"])
        hit = torch.zeros(d.n_rows, H, dtype=torch.bool)
        hit[rows[k0], 0] = True
        assert bool((torch.isnan(out).all(2) == hit).all()) and bool((torch.isnan(out).any(2) == hit).all()), (c, skip)
        keep = ~hit[:, :, None].expand_as(out)
        assert torch.equal(out[keep], fout[keep])
        if "dot" in got:
            assert torch.equal(got["dot"], fin["dot"])      # the dot products do not read the weights


@pytest.mark.parametrize("H,D,hp", [(2, 60, 68), (3, 15, 20), (1, 30, 36), (4, 124, 132)])
def test_bcast_halves_padding_is_zero_behind_nonfinite_columns(H, D, hp):
    """bot_spmm_bcast_halves_f16 writes ZEROS in the columns D .. hpiece - 1 of a head's block whatever the sums are: a NaN and an Inf in
    column 0 of a gathered source row make column 0 of the rows that gather it NaN, and leave the padding of every row zero."""
    g, gd = _graphs()["lanes32"]
    d, dd = g.csc, gd.csc
    r = SC.Recipe()
    c = SC._mk("spmm_bcast_halves", H, D, r, hpiece=hp)
    src = d.indices.long()
    for bad in (float("nan"), float("inf")):
        o = _ops(c, d, g.number_of_src_nodes(), d.eid, "normal", 4, "random")
        o.hscale = torch.tensor([1.0, 1.0])
        o.w = o.w.abs() + 0.5
        o.x[int(src[3]), 0] = bad
        got, name = run(o, dd)
        assert name == c.kernel
        want = SC.halves_expected(o, torch.zeros(d.n_rows, H, D, dtype=torch.float64))
        pad = SC._padding_mask(o)
        assert torch.equal(got["halves"][pad], want[pad]), (H, D, hp, bad)
        assert not bool(torch.isfinite(SC.halves_decode(o, got["halves"])[:, :, 0]).all())


# ------------------------------------------------------------------------------------------------ 6. empty work
@pytest.mark.parametrize("entry", SC.ENTRIES)
def test_empty_work(entry):
    """nnz == 0, every row empty: zeros (the addend for bot_spmm_f32) everywhere, zero halves with their zero padding, absmax 0, and
    nothing written to dot (its guards are intact: run)."""
    g, gd = _graphs()["empty"]
    d, n_cols, own = SC.direction(g, entry)
    dd = SC.direction(gd, entry)[0]
    for H, D, r in ((2, 12, SC.Recipe()), (1, 7, SC.Recipe(pad=1)), (3, 40, SC.Recipe(off=2))):
        if entry == "spmm_dot_halves" and (H < 2 or D < 9 * SC.case_vec(entry, H, D, r)):
            continue
        c = SC._mk(entry, H, D, r, hpiece=(D + 3) // 4 * 4 + 4 if entry == "spmm_bcast_halves" else None)
        for with_addend in (False, True):
            o = _ops(c, d, n_cols, own, "exact", 5, None, with_addend and entry == "spmm")
            got, name = run(o, dd)
            # (an empty w has no address: bot_spmm_f32 sees w == NULL and records the unweighted kernel)
            assert name == (SC.expected_kernel("spmm", H, D, SC.case_vec("spmm", H, D, r), weighted=False) if entry == "spmm" else c.kernel)
            ref = SC.reference(o)
            assert bool((ref["out"] == (o.addend.double() if o.addend is not None else 0)).all())
            assert not SC.check(o, got, ref, True), (c, with_addend)
            assert got.get("dot") is None or got["dot"].numel() == 0


# ------------------------------------------------------------------------------------------------ the figures
def test_zz_report_worst_ratios():
    """Largest error over its derived bound per output kind, over whatever ran before in this process (-s prints it)."""
    print("\nSpMM sweeps, largest error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items())))
    assert all(v <= 1.0 for v in WORST.values())
