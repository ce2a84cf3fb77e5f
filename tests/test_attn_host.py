"""The GAT attention and segment-sum contracts without a GPU: the float64 restatements of tests/attn_cases.py against float64 torch
autograd (so the reference is itself checked), the exact regimes and the seeded cases through the emulated backend
(tests/_oracle_backend.py), the non-vacuity of the derived bounds, the Philox dropout-mask restatement, the non-finite rules on the
emulation, and the entry checks of the three ABI functions.  tests/test_attn_gpu.py holds the kernels to the same restatements."""
import numpy as np
import pytest
import torch

from bot_amd import _C
from tests import _oracle_backend as OB
from tests import attn_cases as AC
from tests.test_sampling_host import philox4x32_10

U = AC.U


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("slope", [0.2, 1.0, 0.0])
def test_restatements_against_fp64_autograd(slope):
    """forward64 / backward64 / segment_sum64 against autograd of softmax(leaky_relu(z)) per row in float64, with all three permutations
    and a keep mask; the logits are kept away from 0, where the leaky ReLU has no derivative."""
    for name, g in AC.graphs()[2:4] + AC.graphs()[-1:]:
        d, H, nnz = g.csc, 3, g.number_of_edges()
        gen = torch.Generator().manual_seed(1)
        el, er, ee, da = (t.double() for t in AC.normal_inputs(g, H, 3))
        eperm, aperm, zperm = (AC.random_perm(nnz, s) for s in (1, 2, 3))
        keep = (torch.rand(nnz, generator=gen) > 0.3).to(torch.uint8)
        rows, src = AC.rows_of(d), d.indices.long()
        leaves = [t.clone().requires_grad_() for t in (el, er, ee)]
        z = leaves[1][rows] + leaves[0][src] + leaves[2][eperm.long()]
        e = torch.where(z > 0, z, z * float(np.float32(slope)))
        kept = keep[eperm.long()] != 0
        m = torch.full((d.n_rows, H), -np.inf, dtype=torch.float64).scatter_reduce(0, rows.view(-1, 1).expand(-1, H)[kept], e.detach()[kept], "amax")
        m = torch.where(torch.isneginf(m), torch.zeros((), dtype=torch.float64), m)
        ex = torch.exp(torch.where(kept.view(-1, 1), e - m[rows], torch.zeros((), dtype=torch.float64))) * kept.view(-1, 1)
        a_pos = ex / torch.zeros(d.n_rows, H, dtype=torch.float64).index_add(0, rows, ex)[rows].clamp(min=1e-300)
        fwd = AC.forward64(d, el, er, ee, eperm, keep, slope, H, aperm)
        a = torch.zeros_like(a_pos)
        a[aperm.long()] = a_pos.detach()
        np.testing.assert_allclose(fwd["a"].numpy(), a.numpy(), rtol=0, atol=1e-14)
        assert bool((fwd["a"][aperm.long()][~kept] == 0).all())
        d_el, d_er, d_ee = torch.autograd.grad(a_pos, leaves, da[aperm.long()])
        bwd = AC.backward64(d, a, da, aperm, zperm, slope, H, gate=fwd["gate"])
        np.testing.assert_allclose(bwd["der"].numpy(), d_er.numpy(), rtol=0, atol=1e-12)
        dz_e = torch.zeros_like(d_ee)
        dz_e[zperm.long()] = d_ee[eperm.long()]                                # d ee[eperm[k]] is dz of position k
        np.testing.assert_allclose(bwd["dz"].numpy(), dz_e.numpy(), rtol=0, atol=1e-12)
        csr, c2c = g.csr, g.csr2csc                                            # d el = the segment sum of dz over the out-edges
        np.testing.assert_allclose(AC.segment_sum64(csr, bwd["dz_pos"], c2c).numpy(), d_el.numpy(), rtol=0, atol=1e-12)
        if H <= 8:
            bits = fwd["zsign"][aperm.long()]
            want = (((z.detach() > 0) & kept.view(-1, 1)).long() << torch.arange(H)).sum(1)
            assert torch.equal(bits.long(), want)


# ------------------------------------------------------------------------------------------------ the emulated backend
@pytest.mark.parametrize("H", [1, 4, 9])
def test_exact_regimes_through_the_emulation(H):
    """The exact regimes' conditions hold for every graph and subset (they are asserted while the inputs are built), and the emulated
    backend gives their results entry for entry."""
    for gi, (name, g) in enumerate(AC.graphs()):
        d, nnz, n_src = g.csc, g.number_of_edges(), g.number_of_src_nodes()
        for si, names in enumerate(AC.SUBSETS):
            seed = 100 * gi + 10 * si + H
            eperm = AC.random_perm(nnz, seed) if si % 2 else None
            aperm = AC.random_perm(nnz, seed + 1) if (si // 2) % 2 else None
            keep = AC.keep_mask(d, (None, "random", "row", "none")[(gi + si) % 4], seed)
            el, er, ee, want, z = AC.equal_logit_inputs(d, n_src, H, names, eperm, keep, seed)
            a = OB.gat_attn_fwd(d, el, er, ee, eperm, keep, 0.25, H, aperm)
            assert torch.equal(a[AC._perm(aperm, nnz)], want), (name, names)
            fwd = AC.forward64(d, el, er, ee, eperm, keep, 0.25, H, aperm)
            assert torch.equal(fwd["a"].float(), a)
        for mode in ("first", "second", "alone", "last", "ties"):
            er, ee, want = AC.spike_inputs(d, H, mode, None, gi + H)
            assert torch.equal(OB.gat_attn_fwd(d, None, er, ee, None, None, 0.25, H, None), want), (name, mode)
        el, er, ee, a, da = AC.integer_backward_inputs(d, n_src, H, gi + H)
        aperm, zperm = AC.random_perm(nnz, gi), AC.random_perm(nnz, gi + 1)
        for slope in (0.25, 1.0, 0.0):
            gate = AC.z32_of(d, el, er, ee, None) > 0
            bwd = AC.backward64(d, a, da, aperm, zperm, slope, H, gate=gate)
            AC.assert_backward_exact(d, bwd)
            dz, der = OB.gat_attn_bwd(d, el, er, ee, None, slope, H, a, da, aperm, zperm, True)
            assert torch.equal(dz.double(), bwd["dz"]) and torch.equal(der.double(), bwd["der"]), (name, slope)
        for dd, perm in ((g.csc, None), (g.csc, g.csc.eid), (g.csr, g.csr2csc)):
            vals = AC.integer_vals(nnz, H, gi)
            assert torch.equal(OB.segment_sum(dd, vals, perm).double(), AC.segment_sum64(dd, vals, perm))
        zs = AC.z32_of(d, *AC.integer_backward_inputs(d, n_src, H, gi + H)[:3], None)
        assert nnz < 30 or bool((zs == 0).any())                               # sums that are exactly 0 occur


@pytest.mark.parametrize("scale", [1.0, 1e3])
def test_seeded_cases_through_the_emulation_under_the_bounds(scale):
    for gi, (name, g) in enumerate(AC.graphs()):
        d, H, nnz = g.csc, 3, g.number_of_edges()
        el, er, ee, da = AC.normal_inputs(g, H, gi, scale)
        eperm = AC.random_perm(nnz, gi)
        a = OB.gat_attn_fwd(d, el, er, ee, eperm, None, 0.2, H, None)
        fwd = AC.forward64(d, el, er, ee, eperm, None, 0.2, H, None)
        fb = AC.forward_bounds(d, fwd)
        assert bool(((a.double() - fwd["a"]).abs() <= fb["a"]).all()), name
        dz, der = OB.gat_attn_bwd(d, el, er, ee, eperm, 0.2, H, a, da, None, None, True)
        bwd = AC.backward64(d, a, da, None, None, 0.2, H, gate=fwd["gate"])
        bb = AC.backward_bounds(d, bwd)
        assert bool(((dz.double() - bwd["dz"]).abs() <= bb["dz"]).all()) and bool(((der.double() - bwd["der"]).abs() <= bb["der"]).all()), name


def test_bounds_are_not_vacuous():
    """For unit-normal el, er, ee on every graph the forward bound stays below 1e-5 relative per weight; a float32 evaluation of the
    restatement in torch passes it; perturbing a single logit by 1e-4 fails it."""
    for gi, (name, g) in enumerate(AC.graphs()):
        d, H, nnz = g.csc, 3, g.number_of_edges()
        el, er, ee, _ = AC.normal_inputs(g, H, 50 + gi)
        fwd = AC.forward64(d, el, er, ee, None, None, 0.2, H, None)
        fb = AC.forward_bounds(d, fwd)
        assert float(torch.expm1(fb["rel"]).max()) < 1e-5, (name, float(fb["rel"].max()))
        rows = AC.rows_of(d)
        z = (er[rows] + el[d.indices.long()]) + ee
        e = torch.where(z > 0, z, z * torch.tensor(0.2))
        m = torch.full((d.n_rows, H), -np.inf).scatter_reduce(0, rows.view(-1, 1).expand(-1, H), e, "amax")
        ex = torch.exp(e - m[rows])
        a32 = ex / torch.zeros(d.n_rows, H).index_add_(0, rows, ex)[rows]
        assert a32.dtype == torch.float32 and bool(((a32.double() - fwd["a"]).abs() <= fb["a"]).all()), name
        k = int(torch.argmax(((fwd["a"][:, 0] > 0.05) & (fwd["a"][:, 0] < 0.9)).float()))
        if not 0.05 < float(fwd["a"][k, 0]) < 0.9:
            continue                                                               # a graph whose rows are all single edges
        ee2 = ee.clone()
        ee2[k, 0] += 1e-4
        moved = AC.forward64(d, el, er, ee2, None, None, 0.2, H, None)["a"]
        assert float((moved[k, 0] - fwd["a"][k, 0]).abs()) > float(fb["a"][k, 0]), name
    assert gi == len(AC.graph_specs()) - 1


# ------------------------------------------------------------------------------------------------ the dropout mask
def test_philox_mask_restatement():
    m1, m2 = AC.drop_mask(500, 9, 0.3, 2 ** 40 + 7), AC.drop_mask(500, 9, 0.3, 2 ** 40 + 7)
    assert torch.equal(m1, m2) and not torch.equal(m1, AC.drop_mask(500, 9, 0.3, 2 ** 40 + 8))
    assert not torch.equal(m1, AC.drop_mask(500, 9, 0.3, 2 ** 40 + 7, seed_offset=1))
    assert AC.drop_seed(5, 3) == (5 + 3 * 0x9E3779B97F4A7C15) % 2 ** 64 and AC.drop_seed(-1) == 2 ** 64 - 1
    seed = 2 ** 33 + 11
    for H in (4, 8, 9, 12):
        mask = AC.drop_mask(300, H, 0.5, seed)
        nq = (H + 3) // 4
        for r in (0, 1, 17, 299):
            for h in range(H):
                w = int(philox4x32_10(seed, np.array([r * nq + h // 4], dtype=np.uint64))[0, h % 4])
                assert bool(mask[r, h]) == (np.float32((w >> 8) * 2.0 ** -24) >= np.float32(0.5)), (H, r, h)
    for p in (0.3, 0.5):
        mask = AC.drop_mask(50000, 4, p, 99)
        n = mask.numel()
        assert n == 200000 and abs(float(mask.double().mean()) - (1 - p)) <= 5 * (p * (1 - p) / n) ** 0.5
    assert AC.drop_scale(0.5) == 2.0


# ------------------------------------------------------------------------------------------------ non-finite logits
def test_nonfinite_rules_on_the_emulation():
    """The three rules of the kernel on the emulated backend: a -inf logit is a dropped edge, a NaN or +inf logit makes its (row, head)
    NaN, a row of nothing but -inf gives zeros."""
    name, g = AC.graphs()[2]
    d, H, nnz = g.csc, 2, g.number_of_edges()
    el, er, ee, _ = AC.normal_inputs(g, H, 4)
    rows = AC.rows_of(d)
    row = int(torch.argmax((AC.degrees(d) == 17).float()))
    b = int(d.indptr[row])
    clean = OB.gat_attn_fwd(d, None, None, ee, None, None, 1.0, H, None)
    for bad in (-np.inf, np.nan, np.inf):
        e2 = ee.clone()
        e2[b, 0] = bad
        got = OB.gat_attn_fwd(d, None, None, e2, None, None, 1.0, H, None)
        want = AC.forward64(d, None, None, e2, None, None, 1.0, H, None)["a"]
        other = torch.ones(nnz, H, dtype=torch.bool)
        other[rows == row, 0] = False
        assert _same(got[other], clean[other])
        if bad == -np.inf:
            assert float(got[b, 0]) == 0 and bool(((got.double() - want).abs() <= 1e-6).all())
            assert abs(float(got[rows == row, 0].sum()) - 1) < 1e-6
        else:
            assert bool(torch.isnan(got[rows == row, 0]).all()) and bool(torch.isnan(want[rows == row, 0]).all())
    e2 = ee.clone()
    e2[rows == row, 1] = -np.inf
    got = OB.gat_attn_fwd(d, None, None, e2, None, None, 1.0, H, None)
    assert bool((got[rows == row, 1] == 0).all()) and _same(got[:, 0], clean[:, 0])
    assert bool((AC.forward64(d, None, None, e2, None, None, 1.0, H, None)["a"][rows == row, 1] == 0).all())


# ------------------------------------------------------------------------------------------------ the C ABI's checks, no GPU
def test_entry_checks_without_gpu():
    lib = _C._lib
    buf = torch.zeros(256)
    p = buf.data_ptr()
    g = lambda k, n, dflt=None: k.get(n, dflt)
    fwd = lambda **k: lib.bot_gat_attn_fwd_f32(p, p, 4, 4, None, g(k, "n_long", 0), 8, g(k, "el"), g(k, "er"), g(k, "ee"), None, None, 0.2,
                                               g(k, "H", 2), g(k, "a", p), None, g(k, "zsign"), g(k, "drop", 0.0), 0, None, g(k, "a_drop"), None)
    bwd = lambda **k: lib.bot_gat_attn_bwd_f32(p, p, 4, 4, None, 0, 8, g(k, "el"), None, None, None, g(k, "slope", 0.2), g(k, "H", 2), g(k, "a", p),
                                               p, None, p, None, None, g(k, "zsign"), g(k, "drop", 0.0), 0, None, None)
    seg = lambda **k: lib.bot_segment_sum_f32(g(k, "indptr", p), g(k, "n", 4), 4, None, g(k, "n_long", 0), g(k, "chunk", 8), g(k, "vals", p), None,
                                              g(k, "W", 2), g(k, "out", p), None)
    assert fwd(el=p, zsign=p, H=9) == -2 and b"zsign holds 8 heads, H=9" in lib.bot_last_error()
    assert fwd(el=p, drop=1.0, a_drop=p) == -2 and b"attn_drop" in lib.bot_last_error()
    assert fwd(el=p, drop=-0.25, a_drop=p) == -2
    assert fwd(el=p, a_drop=p) == -1 and b"a_drop goes with attn_drop" in lib.bot_last_error()
    assert fwd(el=p, drop=0.5) == -1 and b"a_drop goes with attn_drop" in lib.bot_last_error()
    assert fwd() == -1 and b"no logit source" in lib.bot_last_error()
    assert fwd(el=p, a=None) == -1 and fwd(el=p, n_long=1) == -1 and fwd(el=p, H=0) == -2
    assert bwd() == -1 and b"slope != 1 needs zsign" in lib.bot_last_error()
    assert bwd(el=p, zsign=p, H=9) == -2 and b"zsign holds 8 heads" in lib.bot_last_error()
    assert bwd(slope=1.0, drop=1.0) == -2 and b"attn_drop" in lib.bot_last_error()
    assert bwd(el=p, a=None) == -1
    assert seg(W=0) == -2 and seg(chunk=0) == -2 and seg(n=-1) == -2 and seg(n=0) == 0
    assert seg(vals=None) == -1 and seg(out=None) == -1 and seg(indptr=None) == -1 and b"NULL" in lib.bot_last_error()
    assert seg(n_long=1) == -1 and b"long_rows" in lib.bot_last_error()
