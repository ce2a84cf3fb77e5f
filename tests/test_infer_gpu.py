"""The fused inference sweep (csrc/infer.hip, bot_gat_infer_f32) on the MI355X against the float64 restatement of tests/infer_cases.py,
at every instantiation the dispatch can produce (52 names; tests/infer_cases.cases() reaches each): after every call bot_last_kernel()
must be the name the restated dispatch expects; in the exact regimes (equal logits, spikes at a different position per head, plain
sums) the result equals the exactly rounded expectation bit for bit; on seeded inputs at logit scales 1 and 30 every entry stays under
the derived bound; every operand is a view into a guarded allocation (NaN in input padding, a sentinel in output padding and guards
that must come back intact); the absmax by-product of both paths; out as a column block; empty work; run-to-run equality; and the
rules for non-finite logits at every trip width in both row classes.  Called through `_C.gat_infer`.

Measured on the MI355X (run with -s to print them; DESIGN §8 "Inference sweep"): 52 instantiations launched and named (163 cases).
__expf against float64 exp: 1.1042e-07 = 1.85 U at |t| <= 1 (t = -0.987142), 8.0863e-08 per unit of |t| beyond (t = -1.49928); the bound
uses twice those.  Largest error as a fraction of its derived bound, head-major / all-heads layout: flat regime (its long rows whose top
set is not a power of two) 0.502 / 0.287, seeded at logit scale 1 0.935 / 0.923, at scale 30 0.957 / 0.943; plain sums are exact.  On the
library before the running maximum started finite, test_nonfinite_logits_follow_the_stated_rules_fp64 failed at all 11 shapes in its
"trip 1 all -inf" scenario and nowhere else."""
import functools
import types

import numpy as np
import pytest
import torch

from bot_amd import _C
from tests import attn_cases as AC
from tests import infer_cases as IC
from tests import spmm_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda"
WORST = {}
SEEN = set()
FAMILIES = [(fam, v) for fam in ("rows", "heads") for v in (4, 2, 1)]
# one shape per trip width and per way heads share a chunk: head-major LANES 8 / 16 / 32 / 64 / 64 x 2, all-heads HL 16 (four heads a
# chunk), HL 32 (two), HL 64, two chunks a head; and H = 9, 12, 17 for the second and third head tile of the long rows' first pass
SHAPES = ((3, 4), (1, 40), (9, 100), (1, 250), (12, 6), (17, 5), (4, 40), (8, 60), (4, 100), (2, 200), (3, 250))


@functools.lru_cache(maxsize=None)
def _graphs():
    """name -> (CPU graph, device graph), built once; "oneslot": chunk 8 with a row of 7 edges re-planned as a long row of one slot."""
    out = {}
    for name, g in IC.graphs():
        g.create_formats_()
        gd = g.to(DEV)
        gd.create_formats_()
        out[name] = (g, gd.csc)
    g, dd = out["chunk8"]
    one = types.SimpleNamespace(csc=IC.one_slot_plan(g.csc), number_of_src_nodes=g.number_of_src_nodes)
    assert 1 in IC.slots_of(one.csc)[IC.is_long(one.csc)].tolist()
    out["oneslot"] = (one, IC.one_slot_plan(dd))
    return out


def _d(t):
    return None if t is None else t.to(DEV)


def _last():
    return _C._lib.bot_last_kernel().decode()


def _vector(t, off):
    """A [H D] operand `off` floats behind an aligned address, NaN around it."""
    if t is None:
        return None
    buf = torch.full((2 * SC.GUARD + off + t.numel(),), float("nan"), device=DEV)
    view = buf[SC.GUARD + off:SC.GUARD + off + t.numel()]
    view.copy_(t.to(DEV))
    return view


def run(o, dd, absmax=False):
    """One call with every float operand placed under the case's recipe.  -> (result dict of CPU tensors for IC.check, kernel name).
    Asserts the guards of out."""
    r = o.case.recipe
    n = dd.n_rows
    _, x = SC.place(o.x, IC.slab(r), DEV)
    assert x.data_ptr() % 16 == 4 * r.off
    node = SC.Recipe(pad=1 + r.pad % 2, off=r.off)
    el = SC.place(o.el, node, DEV)[1] if o.el is not None else None
    er = SC.place(o.er, node, DEV)[1] if o.er is not None else None
    ee = SC.place(o.ee, SC.Recipe(), DEV)[1] if o.ee is not None else None
    ew = SC.place(o.ew.view(-1, 1), SC.Recipe(), DEV)[1].view(-1) if o.ew is not None else None
    addend = SC.place(o.addend, IC.slab(r, r.ao), DEV)[1] if o.addend is not None else None
    obuf, out = SC.place_out((n, o.H, o.D), IC.slab(r), DEV)
    slots = _C.absmax_slots(DEV) if absmax else None
    _C.gat_infer(dd, x, el, er, ee, ew, o.slope, addend=addend, scale=_vector(o.scale, r.so), shift=_vector(o.shift, r.so), relu=o.relu,
                 out=out, absmax=slots)
    name = _last()
    assert SC.guards_intact(obuf, out, IC.slab(r)), (o.case, "out guards")
    got = {"out": out.cpu().contiguous()}
    if absmax:
        got["absmax"] = float(slots.view(torch.float32).max())
    SEEN.add(name)
    return got, name


def _build(c, g, kind, i, epilogue=True, **kw):
    """The i-th variant of an operand set of `kind` (spike / equal / plain / normal1 / normal30) for case c on CPU graph g."""
    d, n_src = g.csc, g.number_of_src_nodes()
    k = IC.kernel_of(c, d, epilogue)
    names, slope = IC.SUBSETS[i % 7], (0.2, 1.0, 0.0)[(i // 7 + i) % 3]
    if kind in ("spike", "equal"):
        return IC.flat_ops(c, d, n_src, k, kind, kw.pop("names", names), kw.pop("slope", slope), i, ew=i % 2 == 0, epilogue=epilogue, relu=i % 3 == 0, **kw)
    if kind == "plain":
        return IC.plain_ops(c, d, n_src, k, i, ew=i % 2 == 0, epilogue=epilogue, relu=i % 3 == 0)
    return IC.normal_ops(c, d, n_src, k, i, logit_scale=float(kind[6:]), names=kw.pop("names", names if i % 2 else ("el", "er", "ee")), ew=i % 3 != 0,
                         epilogue=epilogue, relu=i % 4 == 0, **kw)


def _shape_case(H, D, r=IC.Recipe()):
    return IC.Case(H, D, r, IC.expected_kernel(H, D, IC.case_vec(H, D, r)))


# ------------------------------------------------------------------------------------------------ 0. the fast exponential
def test_fast_exponential_error_measured_fp64():
    """__expf against float64 exp through the kernel itself: rows of two edges with logits (0, t) and x = (1, 0), (0, 1), so that out is
    the two weights and their ratio is __expf(t) up to the 2 U of the two products by 1 / sum.  4 000 seeded float32 t in [-87, 0] and a
    few set by hand.  The premises of the exact regimes: __expf(0) is 1 (t = 0 gives 0.5 and 0.5) and __expf(-200) is 0.  Prints the
    measured coefficients (c0: |t| <= 1; c1 = error / |t|, |t| > 1) and where they sat; the bound's constants are twice the recorded
    ones, which the measurement must not exceed."""
    import bot_amd
    n = 4000
    t = -87.0 * torch.rand(n, generator=torch.Generator().manual_seed(7))
    t[:6] = torch.tensor([0.0, -200.0, -1.0, -87.0, -0.5, -2.0 ** -20])
    src = torch.cat([torch.zeros(n, dtype=torch.int64), torch.arange(1, n + 1)])
    dst = torch.cat([torch.arange(n), torch.arange(n)])
    g = bot_amd.Graph(src, dst, n + 1, num_dst_nodes=n, chunk=300).to(DEV)
    g.create_formats_()
    el = torch.cat([torch.zeros(1), t]).view(-1, 1)
    x = torch.zeros(n + 1, 1, 2)
    x[0, 0, 0], x[1:, 0, 1] = 1.0, 1.0
    out = _C.gat_infer(g.csc, _d(x), _d(el), slope=1.0).cpu().double().view(n, 2)
    assert out[0].tolist() == [0.5, 0.5] and out[1].tolist() == [1.0, 0.0]
    keep = torch.ones(n, dtype=torch.bool)
    keep[1] = False
    rel = ((out[:, 1] / out[:, 0]) / torch.exp(t.double()) - 1).abs()[keep]
    tk = t.double()[keep].abs()
    near, far = tk <= 1, tk > 1
    c0, c1 = float(rel[near].max()), float((rel[far] / tk[far]).max())
    at0, at1 = float(tk[near][rel[near].argmax()]), float(tk[far][(rel[far] / tk[far]).argmax()])
    print(f"\n__expf: c0 = {c0:.4e} ({c0 / IC.U:.2f} U) at t = -{at0:.6g}; c1 = {c1:.4e} ({c1 / IC.U:.3f} U) per unit at t = -{at1:.6g}; "
          f"largest relative error {float(rel.max()):.4e} at t = -{float(tk[rel.argmax()]):.6g}")
    assert c0 <= IC.EXPF_C0 and c1 <= IC.EXPF_C1, (c0, c1)
    assert bool((rel <= IC.EXPF_C0 + IC.EXPF_C1 * tk).all())


# ------------------------------------------------------------------------------------------------ 1. dispatch
def test_every_instantiation_is_launched_and_named():
    """Every case on the lanes graph without long rows, exact regimes in turn: the recorded kernel is the one the restated dispatch
    expects, the result is exact, and the union of the names is every instantiation the dispatch can produce."""
    g, dd = _graphs()["whole"]
    seen, fails = set(), []
    for i, c in enumerate(IC.cases()):
        o = _build(c, g, ("spike", "equal", "plain")[i % 3], i)
        got, name = run(o, dd)
        assert name == c.kernel == o.kernel, (c, name)
        bad = IC.check(o, got, IC.reference(o))
        if bad:
            fails.append((c, o.regime, bad))
        seen.add(name)
    assert not fails, (len(fails), fails[:8])
    assert seen == set(IC.all_instantiations()) and len(seen) == IC.N_INSTANTIATIONS == 52


def test_width_past_the_tile_is_refused():
    """D = 256 VEC runs (the widest legal width); D = 256 VEC + VEC returns BOT_E_RANGE and writes nothing.  The partials of the long
    rows start 2 n_slots H floats into the workspace, so an odd n_slots H halves VEC: D = 1024 is then past the tile too."""
    g, dd = _graphs()["blocklong"]
    assert g.csc.n_slots % 2 == 1 and IC.kernel_of(_shape_case(1, 1024), g.csc) is None and IC.kernel_of(_shape_case(2, 1024), g.csc) is not None
    with pytest.raises(_C.BotKernelError, match="exceeds"):
        _C.gat_infer(dd, torch.randn(g.number_of_src_nodes(), 1, 1024, device=DEV), torch.randn(g.number_of_src_nodes(), 1, device=DEV))
    g, dd = _graphs()["sweep128"]
    for H, D, v in IC.range_cases():
        c = _shape_case(H, D, IC.Recipe() if D > v * 256 else IC.Recipe(off={4: 0, 2: 2, 1: 1}[v]))
        assert IC.case_vec(H, D, c.recipe) == v
        if c.kernel is None:
            obuf, out = SC.place_out((dd.n_rows, H, D), SC.Recipe(), DEV)
            with pytest.raises(_C.BotKernelError, match="exceeds"):
                _C.gat_infer(dd, torch.randn(g.number_of_src_nodes(), H, D, device=DEV), torch.randn(g.number_of_src_nodes(), H, device=DEV), out=out)
            assert bool((obuf.view(torch.int32) == SC.SENTINEL32).all())
        else:
            o = _build(c, g, "plain", H)
            got, name = run(o, dd)
            assert name == c.kernel and not IC.check(o, got, IC.reference(o)), (H, D)


# ------------------------------------------------------------------------------------------------ 2. both regimes, every case
@pytest.mark.parametrize("family,vec", FAMILIES)
def test_cases_against_fp64(family, vec):
    """The family's cases, each on two graphs in turn (without long rows, default chunk, chunk 8, one slot, and the small graphs): an
    exact regime and a seeded one each, with and without the epilogue operands; the kernel name and the guards after every call; every
    fourth seeded call twice, bitwise equal."""
    graphs = _graphs()
    fails = []
    mine = [(i, c) for i, c in enumerate(IC.cases()) if family in c.kernel and f"<{vec}," in c.kernel]
    assert mine
    for i, c in mine:
        for gi, gname in enumerate((("whole", "default", "chunk8")[i % 3], ("oneslot", "sweep8", "blocklong", "default", "chunk8")[i % 5])):
            j = i + gi
            epilogue = j % 4 != 0
            if IC.kernel_of(c, graphs[gname][0].csc, epilogue) is None:      # D = 256 VEC and an odd n_slots H: refused (the test above)
                gname = "whole"
            g, dd = graphs[gname]
            for kind in (("spike", "equal", "plain")[j % 3], ("normal1", "normal30")[j % 2]):
                o = _build(c, g, kind, j, epilogue)
                got, name = run(o, dd, absmax=j % 2 == 0)
                assert name == o.kernel, (c, gname, name, o.kernel)
                bad = IC.check(o, got, IC.reference(o), WORST, tag=" " + family)
                if bad:
                    fails.append((c, gname, kind, bad))
                if kind.startswith("normal") and j % 4 == 0:
                    again, _ = run(o, dd)
                    assert torch.equal(got["out"].view(torch.int32), again["out"].view(torch.int32)), (c, gname, "two runs differ")
    for f in fails[:8]:
        print("\nFAIL", f)
    assert not fails, (len(fails), fails[:6])


@pytest.mark.parametrize("H,D", SHAPES)
def test_spikes_with_every_subset_and_slope(H, D):
    """All seven subsets of el / er / ee with slopes 0.2, 1 and 0 in turn, spikes and equal logits, on whole rows and on rows of many
    slots: bit for bit.  The spike lies at a different position for each head of a row, so heads that share a chunk need different
    rescale factors in the same trip."""
    fails = []
    for gi, gname in enumerate(("whole", "chunk8")):
        g, dd = _graphs()[gname]
        for i, names in enumerate(IC.SUBSETS):
            for ki, kind in enumerate(("spike", "equal")):
                c = _shape_case(H, D, IC.RECIPES[(i + H) % 4])
                o = _build(c, g, kind, i, i % 2 == 0, names=names, slope=(0.2, 1.0, 0.0)[(i + ki + 2 * gi) % 3])   # every subset meets every slope
                got, name = run(o, dd)
                assert name == o.kernel
                bad = IC.check(o, got, IC.reference(o))
                if bad:
                    fails.append((gname, names, kind, o.slope, bad))
    assert not fails, (len(fails), fails[:6])


# ------------------------------------------------------------------------------------------------ 3. absmax, out as a column block
@pytest.mark.parametrize("H,D", [(3, 40), (3, 250), (1, 40), (9, 7), (17, 5), (5, 300)])
def test_absmax_of_both_paths(H, D):
    """The all-heads path (the kernel's by-product for whole rows, the combine pass's for long ones) and the head-major path (one pass
    per head over a strided out) deliver exactly max |out|: with the largest entry in a long row, in a whole row, and without long rows."""
    r = IC.Recipe(pad=4, hx=4)
    for gname in ("default", "chunk8", "whole"):
        g, dd = _graphs()[gname]
        c = _shape_case(H, D, r)
        for kind, boost in (("plain", None), ("normal1", None), ("normal1", "whole"), ("normal1", "long")):
            o = _build(c, g, kind, 5)
            lng = IC.is_long(g.csc)
            if boost:
                rows = (lng if boost == "long" else ~lng).nonzero().view(-1)
                if not rows.numel():
                    continue
                o.addend[int(rows[len(rows) // 2]), H - 1, D - 1] = 1e4
            got, name = run(o, dd, absmax=True)
            assert name == o.kernel and ("rows" in name) == ((H, D) in ((3, 40), (3, 250)))
            ref = IC.reference(o)
            assert not IC.check(o, got, ref), (gname, kind, boost)
            assert got["absmax"] == float(got["out"].abs().max()) > 0
            if boost:
                assert bool(lng[int(got["out"].abs().amax((1, 2)).argmax())]) == (boost == "long")


def test_out_as_a_column_block_of_a_wider_buffer():
    """out= a column block of a wider [n, 3 H D] buffer: the block equals the contiguous result bit for bit, the rest is untouched."""
    g, dd = _graphs()["default"]
    for H, D in ((3, 40), (1, 40), (9, 7)):
        o = _build(_shape_case(H, D), g, "normal1", 2)
        want, _ = run(o, dd)
        wide = torch.full((dd.n_rows, 3 * H * D), SC.SENTINEL32, dtype=torch.int32, device=DEV).view(torch.float32)
        out = wide[:, H * D:2 * H * D].unflatten(1, (H, D))
        _C.gat_infer(dd, _d(o.x), _d(o.el), _d(o.er), _d(o.ee), _d(o.ew), o.slope, addend=_d(o.addend), scale=_d(o.scale), shift=_d(o.shift), relu=o.relu, out=out)
        w = wide.cpu().view(torch.int32)
        assert torch.equal(w[:, H * D:2 * H * D], want["out"].view(torch.int32).view(dd.n_rows, -1))
        assert bool((w[:, :H * D] == SC.SENTINEL32).all()) and bool((w[:, 2 * H * D:] == SC.SENTINEL32).all())


# ------------------------------------------------------------------------------------------------ 4. empty work
def test_empty_work():
    """nnz == 0 with n_rows > 0: act(addend scale + shift), zeros without the epilogue operands; n_rows == 0 returns cleanly."""
    g, dd = _graphs()["empty"]
    for i, (H, D) in enumerate(((2, 12), (1, 7), (3, 40), (9, 5))):
        for kind in ("plain", "equal"):
            for epilogue in (True, False):
                o = _build(_shape_case(H, D, IC.RECIPES[i]), g, kind, i, epilogue)
                got, name = run(o, dd, absmax=True)
                ref = IC.reference(o)
                v = o.addend.double() * o.scale.double().view(1, H, D) + o.shift.double().view(1, H, D) if epilogue else torch.zeros(dd.n_rows, H, D, dtype=torch.float64)
                assert torch.equal(ref["out"], v.clamp(min=0) if o.relu else v)
                assert name == o.kernel and not IC.check(o, got, ref), (H, D, kind, epilogue)
    z = torch.zeros(8, device=DEV)
    assert _C._lib.bot_gat_infer_f32(None, None, 0, 0, None, 0, None, None, 0, 0, z.data_ptr(), 4, 4, z.data_ptr(), 1, None, 0, None, None, 0.2, 1, 4,
                                     None, 0, 0, None, None, 0, z.data_ptr(), 4, 4, None, None, None) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ 5. non-finite logits
def _nonfinite_ops(H, D, g, seed=9):
    c = _shape_case(H, D)
    return IC.normal_ops(c, g.csc, g.number_of_src_nodes(), IC.kernel_of(c, g.csc, False), seed, names=("ee",), ew=False, epilogue=False, slope=1.0)


@pytest.mark.parametrize("H,D", SHAPES)
def test_nonfinite_logits_follow_the_stated_rules_fp64(H, D):
    """a -inf logit among finite ones is a dropped edge - one anywhere in the row, a whole FIRST trip of them followed by
    finite logits (the running maximum starts finite, so -inf - (-inf) is never formed), a whole second trip; a NaN or +inf logit makes
    its own (row, head) NaN and moves no other bit; a (row, head) of nothing but -inf is NaN.  In head 0 and head H - 1, on whole rows
    (trips of the kernel's own width), on long rows of the default chunk and on rows of many slots."""
    for gname in ("whole", "default", "chunk8"):
        g, dd = _graphs()[gname]
        d = g.csc
        ip, deg = d.indptr.long(), AC.degrees(d)
        base = _nonfinite_ops(H, D, g)
        W = IC.trip_width(base.kernel)
        clean, name = run(base, dd)
        assert name == base.kernel and not IC.check(base, clean, IC.reference(base)), (gname, "clean")
        heads = sorted({0, H - 1})
        multi = [r for r in range(d.n_rows) if deg[r] > W]
        assert multi and any(deg[r] >= 2 for r in range(d.n_rows))
        scenarios = {}
        for where in ("first", "middle", "last"):
            ee = base.ee.clone()
            for r in range(d.n_rows):
                if deg[r] >= 2:
                    ee[int(ip[r]) + {"first": 0, "middle": int(deg[r]) // 2, "last": int(deg[r]) - 1}[where], heads] = -np.inf
            scenarios["one -inf " + where] = ee
        for trip in (0, 1):
            ee = base.ee.clone()
            for r in multi:
                ee[int(ip[r]) + trip * W:min(int(ip[r]) + (trip + 1) * W, int(ip[r + 1])), heads] = -np.inf
            scenarios["trip %d all -inf" % (trip + 1)] = ee
        ee = base.ee.clone()
        for r in multi[::2] + [int((deg == 1).nonzero()[0])]:
            ee[int(ip[r]):int(ip[r + 1]), heads] = -np.inf
        scenarios["all -inf"] = ee
        for bad in (np.nan, np.inf):
            ee = base.ee.clone()
            for r in range(1, d.n_rows, 2):
                if deg[r]:
                    ee[int(ip[r]) + (int(deg[r]) * 2) // 3, heads] = bad
            scenarios[str(bad)] = ee
        fails = []
        for what, ee in scenarios.items():
            o = _nonfinite_ops(H, D, g)
            o.ee = ee
            ref = IC.reference(o)
            got, _ = run(o, dd)
            bad = IC.check(o, got, ref)
            touched = torch.isnan(ref["out"]) | (ref["out"] != IC.reference(base)["out"])
            if not torch.equal(got["out"].view(torch.int32)[~touched], clean["out"].view(torch.int32)[~touched]):
                bad.append("entries of untouched (row, head)s moved")
            if what in ("all -inf", "nan", "inf"):
                assert bool(torch.isnan(ref["out"]).any()) and not bool(torch.isnan(ref["out"][:, 1:H - 1]).any())
            else:
                assert not bool(torch.isnan(ref["out"]).any())
            if bad:
                fails.append((gname, what, bad))
        assert not fails, fails


# ------------------------------------------------------------------------------------------------ the figures
def test_zz_report_worst_ratios():
    """Largest error over its derived bound per regime and layout, over whatever ran before in this process (-s prints it)."""
    print("\nInference sweep, largest error / bound: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(WORST.items()) if isinstance(v, float)))
    for k, v in sorted(WORST.items()):
        if not isinstance(v, float):
            print("   ", k, v)
    print("kernel names seen in this process: %d" % len(SEEN & set(IC.all_instantiations())))
    assert all(v <= 1.0 for v in WORST.values() if isinstance(v, float))
