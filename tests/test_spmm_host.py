"""The SpMM sweeps' contracts without a GPU: the float64 restatements of tests/spmm_cases.py against float64 torch autograd of the dense
formula (so the reference is itself checked), every case of the case list through the emulated backend (tests/_oracle_backend.py) in both
input regimes, the exact regime's premises, the mutants of the restatement (each must break the bit-for-bit comparison AND the derived
bound: the bounds are not vacuous), the case list against the instantiations the dispatchers can produce, and the entry checks of the ABI
functions on paths that return before any launch.  tests/test_spmm_gpu.py holds the kernels to the same restatements."""
import numpy as np
import pytest
import torch

from bot_amd import _C
from tests import _oracle_backend as OB
from tests import attn_cases as AC
from tests import spmm_cases as SC

F64 = torch.float64


def _graph(name):
    return dict(SC.graphs())[name]


def _case(entry, H, D, hpiece=None):
    return SC.Case(entry, H, D, SC.Recipe(), True, False, hpiece, True, "", False)


def emulate(o):
    """The call of o.case.entry on the emulated backend, as the result dict SC.check takes."""
    c, d = o.case, o.d
    got = {}
    if "dot" in c.entry and c.entry != "spmm_dot_bcast":
        dot = torch.full((d.nnz, c.H), 0.0).view(torch.int32).fill_(SC.SENTINEL32).view(torch.float32)
    if "halves" in c.entry:
        ldh, hsh, h2_off, col0, piece = SC.halves_layout(c, d.n_rows)
        hout = torch.full((d.n_rows, ldh), SC.SENTINEL16, dtype=torch.int16).view(torch.float16)
    if c.entry == "spmm":
        got["out"] = OB.spmm(d, o.x, o.w, o.wperm, addend=o.addend)
    elif c.entry == "spmm_dot":
        slots = OB.absmax_slots("cpu")
        got["out"], got["dot"] = OB.spmm_dot(d, o.x, o.w, o.wperm, o.y, dot=dot, absmax=slots)
        got["absmax"] = float(slots.view(torch.float32).max())
    elif c.entry == "spmm_dot_halves":
        got["dot"] = OB.spmm_dot_halves(d, o.x, o.w, o.wperm, o.y, o.hscale, hout[:, col0:], hsh, h2_off, dot=dot)
        got["halves"] = hout.view(torch.int16)
    elif c.entry == "spmm_bcast":
        res = OB.spmm_bcast(d, o.x, o.w, o.wperm, head_outer=c.head_outer)
        got["out"] = res.permute(1, 0, 2).contiguous() if c.head_outer else res
    elif c.entry == "spmm_bcast_halves":
        OB.spmm_bcast_halves(d, o.x, o.w, o.wperm, o.hscale, hout, col0, hsh, h2_off, piece)
        got["halves"] = hout.view(torch.int16)
    else:
        out, got["dot"] = OB.spmm_dot_bcast(d, o.x, o.w, o.wperm, o.y)
        got["out"] = out[:, None, :]
    return got


# ------------------------------------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("name", ["lanes32", "blocklong", "sweep8"])
def test_restatements_against_fp64_autograd(name):
    """spmm <-> spmm_dot and spmm_bcast <-> spmm_dot_bcast are forward and backward of u_mul_e_sum: the restatements against float64
    autograd through the DENSE formula out[:, h] = A_h x[:, h], A_h[dst, src] = the sum of the weights of the parallel edges."""
    g = _graph(name)
    dc, dr, H, D = g.csc, g.csr, 3, 6
    n_src, n_dst, nnz = g.number_of_src_nodes(), g.number_of_dst_nodes(), dc.nnz
    gen = torch.Generator().manual_seed(3)
    w = torch.randn(nnz, H, generator=gen, dtype=F64).requires_grad_()         # in CSC position order
    G = torch.randn(n_dst, H, D, generator=gen, dtype=F64)
    rows, src = AC.rows_of(dc), dc.indices.long()

    def dense(w_):
        A = torch.zeros(H, n_dst, n_src, dtype=F64)
        hh = torch.arange(H)[None, :].expand(nnz, H)
        return A.index_put((hh, rows[:, None].expand(nnz, H), src[:, None].expand(nnz, H)), w_, accumulate=True)

    def ops(case, d, x, y, wperm):
        o = SC.Ops()
        o.case, o.d, o.x, o.w, o.wperm, o.y, o.addend, o.hscale, o.hpiece = case, d, x, w.detach(), wperm, y, None, None, None
        return o
    # heads on the source rows
    x = torch.randn(n_src, H, D, generator=gen, dtype=F64).requires_grad_()
    out = torch.einsum("hrc,chd->rhd", dense(w), x)
    fwd = SC.reference(ops(_case("spmm", H, D), dc, x.detach(), None, None))["out"]
    assert torch.allclose(out, fwd, rtol=1e-12, atol=1e-12)
    dx, dw = torch.autograd.grad((out * G).sum(), (x, w))
    bwd = SC.reference(ops(_case("spmm_dot", H, D), dr, G, x.detach(), g.csr2csc))
    assert torch.allclose(dx, bwd["out"], rtol=1e-12, atol=1e-12) and torch.allclose(dw, bwd["dot"], rtol=1e-12, atol=1e-12)
    # one source row for all heads
    xb = torch.randn(n_src, D, generator=gen, dtype=F64).requires_grad_()
    out = torch.einsum("hrc,cd->rhd", dense(w), xb)
    fwd = SC.reference(ops(_case("spmm_bcast", H, D), dc, xb.detach(), None, None))["out"]
    assert torch.allclose(out, fwd, rtol=1e-12, atol=1e-12)
    dx, dw = torch.autograd.grad((out * G).sum(), (xb, w))
    bwd = SC.reference(ops(_case("spmm_dot_bcast", H, D), dr, G.permute(1, 0, 2).contiguous(), xb.detach(), g.csr2csc))
    assert torch.allclose(dx, bwd["out"][:, 0], rtol=1e-12, atol=1e-12) and torch.allclose(dw, bwd["dot"], rtol=1e-12, atol=1e-12)


def test_halves_encoding_round_trip():
    """The numpy restatement of store_halves: h1 + h2 / 2048 gives z back to 2^-22 |z| (+ the subnormal floor), exactly for values with
    at most 22 significant bits, and the restated layout decodes to what was encoded."""
    rng = np.random.default_rng(0)
    z = (rng.standard_normal(4000) * 2.0 ** rng.integers(-20, 14, 4000)).astype(np.float32)
    h1, h2 = SC.halves_encode(z, 1.0)
    dec = h1.astype(np.float64) + h2.astype(np.float64) / 2048.0
    assert np.all(np.abs(dec - z) <= 2.0 ** -22 * np.abs(z) + 2.0 ** -36)
    ints = rng.integers(-4000, 4001, 4000).astype(np.float32) / 4
    h1, h2 = SC.halves_encode(ints, 2.0)
    assert np.array_equal(h1.astype(np.float64) + h2.astype(np.float64) / 2048.0, ints.astype(np.float64) * 2)


# ------------------------------------------------------------------------------------------------ the case list
def test_case_list_reaches_every_instantiation():
    names = SC.all_instantiations()
    assert len(names) == 265 and len(set(names)) == 265
    assert [len(SC.entry_instantiations(e)) for e in SC.ENTRIES] == [87, 58, 37, 60, 60, 60]
    cases = SC.cases()
    for e in SC.ENTRIES:
        assert {c.kernel for c in cases if c.entry == e} >= set(SC.entry_instantiations(e)), e
    assert {c.kernel for c in cases} == set(names)          # and nothing the dispatchers cannot produce
    for c in cases:                                         # the names follow from the case's own layout
        assert c.kernel == SC.expected_kernel(c.entry, c.H, c.D, SC.case_vec(c.entry, c.H, c.D, c.recipe), c.weighted, c.flat, c.hpiece)
    # every boundary width of every table, per VEC; each recipe; the n_tiles forms; the one-tile limit; hpiece past a table boundary
    for e in SC.ENTRIES:
        for vec in (4, 2, 1):
            got = {-(-c.D // vec) for c in cases if c.entry == e and c.boundary and SC.case_vec(e, c.H, c.D, c.recipe) == vec}
            limit = 257 if e == "spmm" else 256
            want = {L for L in SC.BOUNDARY_L if L <= limit and L * vec <= 1028}
            if e == "spmm_dot_halves":                      # the all-heads layout only: 9 .. 64 lanes, .. 128 below VEC 4
                want = {L for L in want if 8 < L <= (64 if vec == 4 else 128)}
            assert got >= want, (e, vec, sorted(want - got))
    assert {c.recipe.pad for c in cases} >= {0, 1, 2, 4} and {c.recipe.off for c in cases} == {0, 1, 2} and {c.recipe.hx for c in cases} >= {0, 1, 2, 4}
    for vec in (4, 2, 1):                                   # a D divisible by 4 at each of the three widths, through the base offset
        assert any(c.D % 4 == 0 and c.recipe.off == {4: 0, 2: 2, 1: 1}[vec] and c.recipe.pad == 0 and c.recipe.hx == 0 and f"<{vec}," in c.kernel
                   for c in cases)
    assert {True, False} == {c.head_outer for c in cases if c.entry == "spmm_bcast"}
    tiles = {(SC.case_vec("spmm", c.H, c.D, c.recipe), (-(-c.D // SC.case_vec("spmm", c.H, c.D, c.recipe)) + 255) // 256)
             for c in cases if c.entry == "spmm" and "spmm_kernel" in c.kernel}
    assert {t for _, t in tiles} == {1, 2, 3}
    for e in SC.ONE_TILE:
        for vec in (4, 2, 1):
            if "dot_halves" in e:
                continue                                    # 256 lanes a head: beyond the all-heads layout, the only one it has
            assert any(c.entry == e and max(c.D, c.hpiece or 0) == vec * 256 and f"<{vec}," in c.kernel for c in cases), (e, vec)
    for e, H, D, vec in SC.range_cases():
        assert SC.expected_kernel(e, H, D, vec, hpiece=D) is None
    for c in cases:
        if c.entry == "spmm_bcast_halves" and c.hpiece > c.D + 4:
            v = SC.case_vec(c.entry, c.H, c.D, c.recipe)
            assert SC.expected_kernel("spmm_bcast", c.H, c.D, v) != c.kernel            # hpiece crossed a boundary that D did not


def test_graph_classes():
    names = [n for n, _ in SC.graphs()]
    assert names[:3] == ["lanes32", "lanes300", "lanes"] and names[-1] == "empty"
    g = _graph("empty")
    assert g.csc.nnz == 0 and g.csc.n_rows == 5 and g.csr.n_rows == 9 and g.csc.n_items == 5


# ------------------------------------------------------------------------------------------------ the emulation, every case
@pytest.mark.parametrize("entry", SC.ENTRIES)
def test_cases_through_the_emulation(entry):
    """Every case on one of its graphs through tests/_oracle_backend.py: bit for bit in the exact regime (whose premises make_ops asserts),
    under the derived bounds on seeded normal inputs."""
    graphs = dict(SC.graphs())
    worst = {}
    for i, c in enumerate(SC.cases()):
        if c.entry != entry:
            continue
        names = SC.graphs_for(c, i)
        gi = i % len(names)
        g = graphs[names[gi]]
        d, n_cols, own = SC.direction(g, entry)
        wperm, addend, seed = SC.variant(i, gi)
        for regime in ("exact", "normal"):
            o = SC.make_ops(c, d, n_cols, own, regime, seed, wperm, addend and entry == "spmm")
            bad = SC.check(o, emulate(o), SC.reference(o), regime == "exact", worst)
            assert not bad, (c, names[gi], regime, bad)
    assert worst and max(worst.values()) <= 1.0


@pytest.mark.parametrize("entry", SC.ENTRIES)
def test_empty_graph_through_the_emulation(entry):
    g = _graph("empty")
    d, n_cols, own = SC.direction(g, entry)
    c = _case(entry, 2, 12, 16 if entry == "spmm_bcast_halves" else None)
    o = SC.make_ops(c, d, n_cols, own, "exact", 5, None, entry == "spmm")
    ref = SC.reference(o)
    assert bool((ref["out"] == (o.addend.double() if entry == "spmm" else 0)).all()) and (ref["dot"] is None or ref["dot"].numel() == 0)
    assert not SC.check(o, emulate(o), ref, True)


# ------------------------------------------------------------------------------------------------ the mutants
MUTANTS_OF = {"spmm": {1, 2, 3, 4, 5, 6}, "spmm_dot": {1, 2, 3, 4, 5, 7, 9}, "spmm_dot_halves": {1, 2, 3, 4, 5, 7}, "spmm_bcast": {1, 2, 3, 4, 5},
              "spmm_bcast_halves": {1, 2, 3, 4, 5, 8}, "spmm_dot_bcast": {1, 2, 3, 4, 5, 7}}


@pytest.mark.parametrize("entry", SC.ENTRIES)
def test_every_mutant_breaks_both_regimes(entry):
    """The bounds and the bit comparison are not vacuous: each mutant of the restatement that applies to the entry is caught in both
    regimes on the lanes graph with long rows, a random wperm and (bot_spmm_f32) an addend."""
    g = _graph("lanes32")
    d, n_cols, own = SC.direction(g, entry)
    for H, D in ((3, 20), (2, 7)):
        c = _case(entry, H, D, (D + 3) // 4 * 4 + 8 if entry == "spmm_bcast_halves" else None)
        for regime in ("exact", "normal"):
            o = SC.make_ops(c, d, n_cols, own, regime, 17 + H, "random", entry == "spmm")
            got = emulate(o)
            assert not SC.check(o, got, SC.reference(o), regime == "exact")
            assert set(SC.mutants_of(o)) == MUTANTS_OF[entry]
            for m in SC.mutants_of(o):
                assert SC.check(o, got, SC.reference(o, mutant=m), regime == "exact"), (entry, regime, m, SC.MUTANTS[m])


# ------------------------------------------------------------------------------------------------ the C ABI's checks, no GPU
def test_entry_checks_without_gpu():
    """BOT_E_NULL (-1), BOT_E_RANGE (-2) and BOT_E_ALIGN (-3) on the paths that return before a launch, called with CPU pointers."""
    lib = _C._lib
    buf = torch.zeros(4096)
    p = buf.data_ptr()
    assert p % 16 == 0
    g = lambda k, n, dflt=None: k.get(n, dflt)

    def spmm(**k):
        H, D = g(k, "H", 2), g(k, "D", 8)
        return lib.bot_spmm_f32(p, g(k, "indices", p), g(k, "n", 4), 4, g(k, "items", p), 4, None, None, g(k, "n_long", 0), g(k, "x", p),
                                g(k, "ldx", H * D), g(k, "hsx", D), p, None, H, D, g(k, "out", p), g(k, "ldo", H * D), g(k, "hso", D),
                                g(k, "addend"), g(k, "lda", H * D), g(k, "hsa", D), None, None)

    def dot(**k):
        H, D = g(k, "H", 2), g(k, "D", 8)
        return lib.bot_spmm_dot_f32(p, p, g(k, "n", 4), 4, p, 4, None, None, g(k, "n_long", 0), g(k, "x", p), g(k, "ldx", H * D), D, g(k, "w", p), None,
                                    g(k, "y", p), g(k, "ldy", H * D), D, H, D, g(k, "out", p), H * D, D, g(k, "dot", p), None, None, None)

    def dot_halves(**k):
        H, D = g(k, "H", 2), g(k, "D", 8)
        hsh = (D + 3) // 4 * 4
        return lib.bot_spmm_dot_halves_f16(p, p, g(k, "n", 4), 4, p, 4, None, None, g(k, "n_long", 0), p, g(k, "ldx", H * D), D, p, None, p, H * D, D, H, D,
                                           g(k, "hscale", p), g(k, "hout", p), 2 * H * hsh, hsh, g(k, "h2_off", H * hsh), p, None, None)

    def bcast(**k):
        H, D = g(k, "H", 2), g(k, "D", 8)
        return lib.bot_spmm_bcast_f32(p, p, g(k, "n", 4), 4, p, 4, None, None, g(k, "n_long", 0), g(k, "x", p), g(k, "ldx", D), g(k, "w", p), None, H, D,
                                      g(k, "out", p), g(k, "ldo", H * D), D, None, None)

    def bcast_halves(**k):
        H, D = g(k, "H", 2), g(k, "D", 8)
        hp = g(k, "hpiece", (D + 3) // 4 * 4)
        return lib.bot_spmm_bcast_halves_f16(p, p, g(k, "n", 4), 4, p, 4, None, None, g(k, "n_long", 0), p, g(k, "ldx", D), p, None, H, D, g(k, "hscale", p),
                                             g(k, "hout", p), 2 * H * hp, hp, H * hp, hp, None, None)

    def dot_bcast(**k):
        H, D = g(k, "H", 2), g(k, "D", 8)
        return lib.bot_spmm_dot_bcast_f32(p, p, g(k, "n", 4), 4, p, 4, None, None, g(k, "n_long", 0), p, g(k, "ldx", D), 4 * D, p, None, g(k, "y", p), D, H, D,
                                          g(k, "out", p), g(k, "ldo", D), g(k, "dot", p), None, None)

    err = lib.bot_last_error
    # one launch tile: D = vec * 256 + vec at each vector width (the base offsets 4 and 8 bytes bring a D divisible by 4 down to 1 and 2)
    for fn in (dot, dot_halves, dot_bcast, bcast, bcast_halves):
        assert fn(D=514) == -2 and b"exceeds" in err(), fn.__name__
        assert fn(D=257) == -2 and b"exceeds" in err(), fn.__name__
    assert dot(D=1028) == -2 and b"exceeds the 1024 floats" in err()
    assert dot(D=516, x=p + 8) == -2 and b"exceeds the 512 floats" in err()
    assert dot(D=260, x=p + 4) == -2 and b"exceeds the 256 floats" in err()
    assert dot_halves(D=1028) == -2 and b"exceeds one launch tile" in err()
    assert bcast_halves(D=500, hpiece=516, ldx=502) == -2 and b"hpiece=516 exceeds" in err()
    for fn in (bcast, bcast_halves, dot_bcast):
        assert fn(D=1028) == -2 and fn(H=5) == -2 and b"H=5 (1..4)" in err() and fn(H=0) == -2, fn.__name__
    assert dot_halves(H=1) == -2 and b"needs H >= 2" in err()
    # strides smaller than the slab
    assert spmm(ldx=15) == -2 and b"strides smaller than the slab" in err()
    assert spmm(hsx=7) == -2 and spmm(ldo=15) == -2 and spmm(hso=7) == -2
    assert spmm(addend=p, lda=15) == -2 and b"addend strides" in err() and spmm(addend=p, hsa=7) == -2
    assert dot(ldx=15) == -2 and dot(ldy=15) == -2 and b"strides smaller than the slab" in err()
    assert dot_halves(ldx=15) == -2 and b"strides smaller than the slab" in err()
    assert dot_halves(h2_off=8) == -2 and b"h2_off=8" in err()
    assert bcast(ldx=7) == -2 and bcast(ldo=7) == -2 and bcast_halves(ldx=7) == -2 and bcast_halves(hpiece=6) == -2
    assert dot_bcast(ldx=7) == -2 and dot_bcast(ldo=7) == -2
    assert spmm(H=0) == -2 and spmm(D=0) == -2 and spmm(n=-1) == -2 and dot(H=0) == -2
    # NULL
    assert spmm(x=None) == -1 and spmm(out=None) == -1 and spmm(items=None) == -1 and spmm(indices=None) == -1
    assert spmm(n_long=1) == -1 and b"long rows need" in err()
    assert dot(x=None) == -1 and dot(y=None) == -1 and dot(w=None) == -1 and dot(dot=None) == -1 and dot(n_long=1) == -1
    assert dot_halves(hout=None) == -1 and dot_halves(hscale=None) == -1 and dot_halves(n_long=1) == -1
    assert bcast(x=None) == -1 and bcast(w=None) == -1 and bcast(out=None) == -1 and bcast(n_long=1) == -1
    assert bcast_halves(hout=None) == -1 and bcast_halves(hscale=None) == -1 and bcast_halves(n_long=1) == -1
    assert dot_bcast(y=None) == -1 and dot_bcast(dot=None) == -1 and dot_bcast(out=None) == -1 and dot_bcast(n_long=1) == -1
    # alignment
    assert spmm(x=p + 2) == -3 and b"misaligned" in err() and spmm(out=p + 1) == -3 and spmm(items=p + 4) == -3
    assert bcast_halves(hout=p + 4) == -2
    # nothing to do
    assert spmm(n=0) == 0 and dot(n=0) == 0 and bcast(n=0) == 0 and bcast_halves(n=0) == 0 and dot_bcast(n=0) == 0 and dot_halves(n=0) == 0
