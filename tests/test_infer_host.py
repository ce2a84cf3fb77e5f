"""The fused inference sweep's contract without a GPU: the float64 restatement of tests/infer_cases.py against a row-by-row float64
torch.softmax formulation and against the emulated backend (tests/_oracle_backend.gat_infer), the exact regimes' premises and their
expected values against the restatement, the restated dispatch against the 52 names counted from csrc/infer.hip and the case list that
reaches them, the mutants of the restatement (each must break an exact regime AND the derived bound on seeded inputs: the checks are not
vacuous), and the entry checks of bot_gat_infer_f32 on paths that return before any launch.  tests/test_infer_gpu.py holds the kernels
to the same restatement."""
import ctypes

import numpy as np
import pytest
import torch

from bot_amd import _C
from tests import _oracle_backend as OB
from tests import attn_cases as AC
from tests import infer_cases as IC

F64 = torch.float64


def _graph(name):
    return dict(IC.graphs())[name]


def _case(H, D):
    return IC.Case(H, D, IC.Recipe(), IC.expected_kernel(H, D, IC.case_vec(H, D, IC.Recipe())))


def _ops(name, H, D, kind, seed=3, **kw):
    g = _graph(name)
    c = _case(H, D)
    k = IC.kernel_of(c, g.csc)
    n_src = g.number_of_src_nodes()
    if kind == "normal":
        return IC.normal_ops(c, g.csc, n_src, k, seed, **kw)
    if kind == "plain":
        return IC.plain_ops(c, g.csc, n_src, k, seed, **kw)
    return IC.flat_ops(c, g.csc, n_src, k, kind, kw.pop("names", ("el", "er", "ee")), kw.pop("slope", 0.2), seed, **kw)


def _as_got(o, ref, mutated=None):
    """What a kernel that computed `mutated` (or the restatement itself) would hand to IC.check: float32 out, and in the exact regimes
    the exactly rounded values wherever the restatement is untouched by the mutation."""
    src = ref if mutated is None else mutated
    out = src["out"].float()
    if o.regime in ("flat", "plain"):
        exp, mask = IC.exact_expected(o)
        same = (src["out"] == ref["out"]) & mask
        out = torch.where(same, exp, out)
    return {"out": out, "absmax": src["absmax"] if mutated is not None and mutated["mutant"] == 10 else float(torch.nan_to_num(out.abs()).max())}


# ------------------------------------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("name", ["default", "chunk8", "blocklong", "empty"])
def test_restatement_against_row_by_row_fp64_and_the_emulated_backend(name):
    """out row by row with torch.softmax in float64 (no scatter, no running maximum), every optional operand present and absent; and
    the emulated backend's float32 result within 1e-5 of the largest entry."""
    g = _graph(name)
    d = g.csc
    ip, src = d.indptr.long(), d.indices.long()
    for i, (names, ew, epi, relu) in enumerate(((("el", "er", "ee"), True, True, True), (("el",), False, False, False), (("el", "ee"), True, False, True),
                                                (("er",), False, True, False))):
        o = _ops(name, 3, 5, "normal", seed=i, names=names, ew=ew, epilogue=epi, relu=relu)
        ref = IC.reference(o)["out"]
        want = torch.zeros(d.n_rows, 3, 5, dtype=F64)
        for r in range(d.n_rows):
            b, e = int(ip[r]), int(ip[r + 1])
            if e > b:
                z = o.el.double()[src[b:e]] + (o.er.double()[r] if o.er is not None else 0) + (o.ee.double()[b:e] if o.ee is not None else 0)
                a = torch.softmax(torch.nn.functional.leaky_relu(z, float(np.float32(o.slope))), 0)
                if o.ew is not None:
                    a = a * o.ew.double()[b:e, None]
                want[r] = (a[:, :, None] * o.x.double()[src[b:e]]).sum(0)
        if epi:
            want = (want + o.addend.double()) * o.scale.double().view(1, 3, 5) + o.shift.double().view(1, 3, 5)
        want = want.clamp(min=0) if relu else want
        assert torch.allclose(ref, want, rtol=1e-12, atol=1e-12), (name, names)
        emu = OB.gat_infer(d, o.x, o.el, o.er, o.ee, o.ew, o.slope, addend=o.addend, scale=o.scale, shift=o.shift, relu=relu)
        assert float((emu.double() - ref).abs().max() if ref.numel() else 0) <= 1e-5 * max(float(ref.abs().max()) if ref.numel() else 0, 1.0)
    o = _ops(name, 2, 6, "plain", ew=True)
    emu = OB.gat_infer(d, o.x, None, None, None, o.ew, addend=o.addend, scale=o.scale, shift=o.shift)
    assert torch.equal(emu.double(), IC.reference(o)["out"])                    # exact regime: the float32 emulation has nothing to round


def test_nonfinite_rules_of_the_restatement():
    """A -inf logit is a dropped edge, NaN / +inf poison their (row, head), all -inf is NaN, an empty row is the epilogue of zero."""
    o = _ops("whole", 2, 3, "normal", names=("ee",), ew=False, epilogue=False)
    d = o.d
    ip = d.indptr.long()
    r = int((AC.degrees(d) == 9).nonzero()[0])
    b = int(ip[r])
    base = IC.reference(o)["out"]
    o.ee[b, 0] = -np.inf
    got = IC.reference(o)["out"]
    z = o.ee.double()[b + 1:b + 9, 0]
    a = torch.softmax(torch.where(z > 0, z, z * float(np.float32(0.2))), 0)
    assert torch.allclose(got[r, 0], (a[:, None] * o.x.double()[d.indices.long()[b + 1:b + 9], 0]).sum(0), rtol=1e-12, atol=1e-12)
    keep = torch.ones(d.n_rows, 2, dtype=torch.bool)
    keep[r, 0] = False
    assert torch.equal(got[keep], base[keep])
    for bad in (np.nan, np.inf):
        o.ee[b, 0] = bad
        got = IC.reference(o)["out"]
        assert bool(torch.isnan(got[r, 0]).all()) and torch.equal(got[keep], base[keep])
    o.ee[b:b + 9, 0] = -np.inf
    got = IC.reference(o)["out"]
    assert bool(torch.isnan(got[r, 0]).all()) and torch.equal(got[keep], base[keep]) and bool((got[0] == 0).all())


# ------------------------------------------------------------------------------------------------ the exact regimes
@pytest.mark.parametrize("name", ["whole", "default", "chunk8", "sweep8"])
def test_exact_premises_and_expected_values(name):
    """The builders assert their premises (assert_exact); the exactly rounded expectation lies within the bound of the float64
    restatement everywhere, is exact on every whole row, and on the spikes is ew x of the spike's own source."""
    d = _graph(name).csc
    for H, D in ((1, 4), (3, 12), (5, 9)):
        for i, names in enumerate(IC.SUBSETS):
            for mode in ("equal", "spike"):
                o = _ops(name, H, D, mode, seed=i, names=names, slope=(0.2, 1.0, 0.0)[i % 3], ew=i % 2 == 0, epilogue=i % 3 != 0, relu=i % 4 == 0)
                ref = IC.reference(o)
                exp, mask = IC.exact_expected(o)
                assert bool(((exp.double() - ref["out"]).abs() <= IC.out_bound(o, ref)).all()), (name, H, names, mode)
                assert bool(mask[~IC.is_long(d)].all()) and (mode == "equal" or "ee" not in names or bool(mask.all()))
                if mode == "spike" and "ee" in names and o.addend is None and not o.relu:
                    pos = IC.spike_positions(d, H, IC.trip_width(o.kernel))
                    for r in (1, d.n_rows - 1):
                        for h in range(H):
                            k = int(pos[r, h])
                            assert torch.equal(exp[r, h], o.x[int(d.indices[k]), h] * (o.ew[k] if o.ew is not None else 1) + 0.0)
        o = _ops(name, 2, 7, "plain", ew=True)
        assert IC.exact_expected(o)[1].all() and torch.equal(IC.exact_expected(o)[0].double(), IC.reference(o)["out"] + 0.0)


def test_spikes_ask_for_different_rescales_in_one_trip():
    """In a row of more than one trip the heads' spikes lie in different trips, so heads that share a 64-lane chunk need different
    factors in the same trip; over the rows every head meets every kind of position."""
    d = _graph("whole").csc
    pos, ip = IC.spike_positions(d, 4, 64), d.indptr.long()
    r = int(AC.degrees(d).argmax())
    trips = {int((pos[r, h] - ip[r]) // 64) for h in range(4)}
    assert len(trips) >= 3
    kinds = {(h, int((h + r) % 5)) for h in range(4) for r in range(d.n_rows)}
    assert len(kinds) == 20


# ------------------------------------------------------------------------------------------------ the dispatch
def test_case_list_reaches_every_instantiation():
    names = IC.all_instantiations()
    assert len(names) == len(set(names)) == IC.N_INSTANTIATIONS == 52
    assert sum("rows" in n for n in names) == 31 and sum("heads" in n for n in names) == 21
    cases = IC.cases()
    assert {c.kernel for c in cases} == set(names)
    whole = _graph("whole").csc
    for c in cases:
        assert c.kernel == IC.kernel_of(c, whole) == IC.expected_kernel(c.H, c.D, IC.case_vec(c.H, c.D, c.recipe))
    # the whole domain maps into the counted names: every H, every width up to the tile, every VEC
    seen = {IC.expected_kernel(H, D, v) for H in range(1, 19) for v in (4, 2, 1) for D in range(v, v * 256 + 1, v)}
    assert seen == set(names)
    assert {c.H for c in cases} == set(IC.HEADS) and {c.recipe for c in cases} == set(IC.RECIPES)
    for v in (4, 2, 1):
        assert {-(-c.D // v) for c in cases if f"<{v}," in c.kernel} >= set(IC.BOUNDARY_L), v
    # padded head slots and full chunks of the all-heads layout: the smallest and the largest H of every (HL, NCHUNK)
    for n in names:
        if "rows" in n and n.endswith(",1>"):
            v, hl, nc, _ = (int(t) for t in n.split("<")[1][:-1].split(","))
            hs = {c.H for c in cases if c.kernel == n}
            fit = [H for H in range(2, 9) if (H * hl + 63) // 64 == nc]
            assert min(fit) in hs and max(fit) in hs, (n, hs)
    for H, D, v in IC.range_cases():
        assert (IC.expected_kernel(H, D, v) is None) == (D > v * 256)
    # the slot count decides VEC with the rest: an odd n_slots H leaves the partials 8 bytes off a 16-byte boundary
    assert IC.case_vec(3, 8, IC.Recipe(), n_slots=1) == 2 and IC.case_vec(3, 8, IC.Recipe(), n_slots=2) == 4 and IC.case_vec(2, 8, IC.Recipe(), n_slots=1) == 4


# ------------------------------------------------------------------------------------------------ the mutants
MUTANT_SETUPS = {1: ("chunk8", "spike", {}), 2: ("whole", "spike", dict(names=("el", "ee"))), 3: ("default", "spike", dict(names=("el", "er"))),
                 4: ("default", "spike", {}), 5: ("whole", "spike", dict(ew=True)), 6: ("default", "equal", {}), 7: ("chunk8", "equal", {}),
                 8: ("default", "plain", {}), 9: ("whole", "plain", dict(relu=True)), 10: ("chunk8", "plain", {})}


@pytest.mark.parametrize("mutant", sorted(IC.MUTANTS))
def test_mutants_break_both_regimes(mutant):
    """The unmutated restatement passes IC.check in an exact regime and on seeded inputs; the mutant fails both."""
    name, kind, kw = MUTANT_SETUPS[mutant]
    for regime in (kind, "normal"):
        kw2 = dict(kw, relu=True) if mutant == 9 else dict(kw)
        for seed in range(mutant, mutant + 20):
            o = _ops(name, 4, 12, regime, seed=seed, **kw2)
            ref = IC.reference(o)
            # mutant 10's premise: the largest entry lies in a long row (the first seed for which it does)
            if mutant != 10 or bool(IC.is_long(o.d)[int(ref["out"].abs().amax((1, 2)).argmax())]):
                break
        else:
            raise AssertionError("no seed puts the largest entry into a long row")
        assert mutant in IC.mutants_of(o), (mutant, regime)
        assert not IC.check(o, _as_got(o, ref), ref), (mutant, regime, "the restatement itself")
        mut = IC.reference(o, mutant)
        assert IC.check(o, _as_got(o, ref, mut), ref), (mutant, regime, IC.MUTANTS[mutant])


# ------------------------------------------------------------------------------------------------ the entry checks
def _entry(**kw):
    """bot_gat_infer_f32 on host memory with ONE thing wrong, so that it returns before any launch.  -> (rc, message)."""
    H, D, n, nnz = kw.pop("H", 2), kw.pop("D", 4), 4, 6
    buf = {k: torch.zeros(4096, dtype=torch.float32) for k in ("x", "el", "er", "ee", "out", "ws")}
    ints = torch.zeros(256, dtype=torch.int32)
    a = dict(indptr=ints.data_ptr(), indices=ints.data_ptr(), n_rows=n, nnz=nnz, items=ints.data_ptr(), n_items=n, long_rows=None, long_ptr=None,
             n_long=0, n_slots=0, x=buf["x"].data_ptr(), ldx=H * D, hsx=D, el=buf["el"].data_ptr(), ldel=H, er=None, lder=0, ee=None, ew=None,
             slope=0.2, H=H, D=D, addend=None, lda=0, hsa=0, scale=None, shift=None, relu=0, out=buf["out"].data_ptr(), ldo=H * D, hso=D,
             workspace=None, absmax=None, stream=None)
    for k, v in kw.items():
        a[k] = buf[v].data_ptr() if isinstance(v, str) else v
    rc = _C._lib.bot_gat_infer_f32(*[ctypes.c_float(v) if k == "slope" else v for k, v in a.items()])
    return rc, _C._lib.bot_last_error().decode()


def test_entry_checks_return_before_any_launch():
    NULL, RANGE = -1, -2
    for kw, code, word in ((dict(el=None, er="er", lder=2), NULL, "without el"), (dict(el=None, ee="ee"), NULL, "without el"),
                           (dict(ldel=1), RANGE, "ldel"), (dict(er="er", lder=1), RANGE, "lder"),
                           (dict(ldx=7), RANGE, "strides smaller"), (dict(hsx=3), RANGE, "strides smaller"), (dict(ldo=7), RANGE, "strides smaller"),
                           (dict(hso=3), RANGE, "strides smaller"), (dict(addend="x", lda=7, hsa=4), RANGE, "addend strides"),
                           (dict(addend="x", lda=8, hsa=3), RANGE, "addend strides"),
                           (dict(n_long=1, n_slots=2, long_rows=None, long_ptr=None), NULL, "long rows need"),
                           (dict(n_long=1, n_slots=2, long_rows="x", long_ptr="x", workspace=None), NULL, "long rows need"),
                           (dict(H=0), RANGE, "H=0"), (dict(D=0), RANGE, "D=0"), (dict(n_rows=-1), RANGE, "negative"),
                           (dict(x=None), NULL, "NULL"), (dict(out=None), NULL, "NULL"), (dict(indices=None), NULL, "indices")):
        rc, msg = _entry(**kw)
        assert rc == code and word in msg, (kw, rc, msg)
    # D past the tile of the VEC the operands allow: 1028 floats at VEC 4, 514 at VEC 2 (an 8-byte pitch), 257 at VEC 1
    for D, extra in ((1028, {}), (514, {}), (257, {})):
        rc, msg = _entry(H=1, D=D, ldx=D, ldo=D, hsx=D, hso=D, **extra)
        assert rc == RANGE and "exceeds" in msg, (D, rc, msg)
    for H, D, v in IC.range_cases():
        if IC.expected_kernel(H, D, v) is None:
            assert IC.case_vec(H, D, IC.Recipe()) == v                       # D = 1028, 514, 257: the width itself leaves VEC = v
            rc, msg = _entry(H=H, D=D, ldx=H * D, ldo=H * D, hsx=D, hso=D, ldel=H)
            assert rc == RANGE and ("%d floats" % (v * 256)) in msg, (H, D, v, rc, msg)
    # nothing to do: n_rows == 0 returns 0 whatever else is passed
    assert _entry(n_rows=0, x=None, out=None)[0] == 0
