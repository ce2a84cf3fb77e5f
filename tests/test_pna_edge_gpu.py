"""PNA with edge features on the MI355X: the fused sweep and its persistent backward (csrc/spmm_pna_edge.hip) and
`ops.pna_aggregate_edge` against the float64 restatement (tests/pna_edge_cases.py) - byte for byte against the edge-less sweeps where
the contract says so (weight = 0; constant ef within a row), entry for entry where the arithmetic is exact (small integers), inside
rounding bounds derived from the kernel's own order otherwise - `nn.EdgePNAConv` / `nn.EdgePNA` against their float64 restatements
under the suite's criteria (tests/parity_cases.py), and one train step / one sampled epoch of `workloads.build_pna_edge`.

The rounding bounds (tests/pna_edge_cases.py `bounds`; u = 2^-24, D = max_k (|a_k - a_0| + |c_k - c_0|), C_k = sum_j |ef_kj wt_jf|):
    mean     (deg + 4) u (D + |a_0| + |c_0| + |b|) + 2 K u max C
    sum      (deg + 4) u (sum_k (|a_k| + |c_k|) + deg (|a_0| + |c_0| + |b|)) + 2 K u (sum_k C_k + deg C_0)
    var      (3 deg + 16) u D^2 + 8 K u D max C;  std is compared as out^2 - 1e-30 against var, plus 4 u out^2
    max/min  (K + 3) u (max_k (|a_k| + C_k) + |b|)
The SAME bounds hold for a + 1000: the split pivot's point (tests/test_pna_edge_host.py shows a single pivot failing them)."""
import numpy as np
import pytest
import torch

from bot_amd import _C, ops, workloads
from bot_amd import nn as bnn
from bot_amd.sampling import MultiLayerNeighborSampler, NodeDataLoader
from tests import pna_cases as PC
from tests import pna_edge_cases as PE
from tests import sage_cases as SG
from tests.parity_cases import fwd_close, grad_close
from tests.test_sage_gpu import _block, _graphs, _hub, _parent, _same_bytes, _slab

pytestmark = pytest.mark.gpu
DEV = "cuda"
WIDTHS = (1, 3, 4, 5, 64, 65, 256, 1000)     # every vector width and group size; 1000 walks feature tiles
KS = (1, 3, 8, 16)                           # 8 and 16 read ef rows with 16-byte loads; 1 .. 4, 5 .. 8, 9 .. 16 are the three instances
EXACT = ("sum", "max", "min")
ALL6 = ("mean", "sum", "max", "min", "std", "var")
U = PC.U32


def _ks(F_):
    return KS if F_ in (4, 64, 256) else (8, KS[F_ % 4])


def _towers(F_):
    return [F_ // t for t in (1, 2, 4) if F_ % t == 0]


def _ones(g):
    return torch.ones((1, g.number_of_dst_nodes()), device=DEV)


def _eperm(g):
    return ops._csc_edge_rows(g)


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _forward(g, a, b, ef, w, aggs, scale, Ft, pad=0):
    """One `_C.spmm_pna_edge` call on operands inside buffers `pad` columns wider than their rows -> device (out, saved, sarg), after
    the checks that nothing was written beyond a row and that a second call gives the same bytes."""
    n, F_ = g.number_of_dst_nodes(), a.shape[1]
    W = scale.shape[0] * len(aggs) * F_
    ad, bd = _slab(a, pad), None if b is None else _slab(b, pad)
    out = torch.full((n, W + pad), 9.0, device=DEV)[:, :W] if pad else None
    saved = torch.full((n, 2 * F_ + pad), 9.0, device=DEV)[:, :2 * F_] if pad else None
    sarg = torch.full((n, 2 * F_ + pad), 9, dtype=torch.int32, device=DEV)[:, :2 * F_] if pad else None
    o, s, p = _C.spmm_pna_edge(g.csc, ad, bd, ef, w, aggs, scale, Ft, want_saved=True, eperm=_eperm(g), out=out, saved=saved, sarg=sarg)
    if pad:
        assert o.data_ptr() == out.data_ptr() and s.data_ptr() == saved.data_ptr() and p.data_ptr() == sarg.data_ptr()
        assert bool((o._base[:, W:] == 9.0).all()) and bool((s._base[:, 2 * F_:] == 9.0).all()) and bool((p._base[:, 2 * F_:] == 9).all())
    o2, s2, p2 = _C.spmm_pna_edge(g.csc, ad, bd, ef, w, aggs, scale, Ft, want_saved=True, eperm=_eperm(g))
    assert _same_bytes(o2, o) and _same_bytes(s2, s) and torch.equal(p2, p)
    return o, s, p


def _backward(g, a, ef, w, aggs, dout, saved, sarg, scale, Ft, pad=0, **kw):
    """prep + `_C.spmm_pna_edge_bwd` -> (da, db, dweight); with `pad` da lies inside a wider buffer that must stay untouched."""
    n_src, F_ = g.number_of_src_nodes(), a.shape[1]
    rec, db = _C.pna_bwd_prep(g.csc, dout, aggs, saved, sarg, scale, Ft)
    dx = torch.full((n_src, F_ + pad), 9.0, device=DEV)[:, :F_] if pad else None
    da, dw = _C.spmm_pna_edge_bwd(g.csr, g.csr2csc, a, ef, w, rec, aggs, eperm=g.csr.eid, out=dx, **kw)
    if pad and da is not None:
        assert da.data_ptr() == dx.data_ptr() and bool((da._base[:, F_:] == 9.0).all())
    return da, db, dw


# ------------------------------------------------------------------------------------------------ 1. weight = 0: the edge-less sweeps
@pytest.mark.parametrize("F_", WIDTHS)
def test_zero_weight_gives_the_edge_less_sweeps_results(F_):
    """weight = 0: c = 0, so out, saved, sarg and da are `_C.spmm_pna` / `_C.spmm_pna_bwd` on the same a and b, value for value (the
    two differ at most in the sign of a zero: a + 0 is +0 for a = -0)."""
    for name, g in _graphs():
        rng = np.random.default_rng(7 * F_ + len(name))
        a = rng.standard_normal((g.number_of_src_nodes(), F_)).astype(np.float32)
        b = rng.standard_normal((g.number_of_dst_nodes(), F_)).astype(np.float32)
        scale = ops.pna_scale_table(g, PC.SCALERS3, 1.3)
        for K in _ks(F_):
            ef = _dev(rng.standard_normal((g.number_of_edges(), K)).astype(np.float32))
            w = torch.zeros((F_, K), device=DEV)
            for pad in (0, 3, 4):
                for Ft in _towers(F_):
                    o, s, p = _forward(g, a, b, ef, w, ALL6, scale, Ft, pad)
                    assert "spmm_pna_edge" in _C._lib.bot_last_kernel().decode()
                    ad, bd = _slab(a, pad), _slab(b, pad)
                    o0, s0, p0 = _C.spmm_pna(g.csc, ad, bd, ALL6, scale, Ft, want_saved=True)
                    assert torch.equal(o, o0) and torch.equal(s, s0) and torch.equal(p, p0), (name, F_, K, pad, Ft)
                    dout = torch.randn(o0.shape, generator=torch.Generator().manual_seed(K)).to(DEV)
                    da, db, dw = _backward(g, ad, ef, w, ALL6, dout, s, p, scale, Ft, pad)
                    assert "spmm_pna_edge_bwd_kernel<dx,dw," in _C._lib.bot_last_kernel().decode()
                    rec, db0 = _C.pna_bwd_prep(g.csc, dout, ALL6, s0, p0, scale, Ft)
                    assert torch.equal(da, _C.spmm_pna_bwd(g.csr, g.csr2csc, ad, rec, ALL6)) and torch.equal(db, db0), (name, F_, K, pad, Ft)
                    assert dw.shape == (F_, K) and bool(torch.isfinite(dw).all())


def test_last_kernel_names_the_new_kernels():
    name, g = _graphs()[4]                                             # long rows: the combine runs behind the sweep
    a = torch.randn(g.number_of_src_nodes(), 8, device=DEV)
    ef, w = torch.randn(g.number_of_edges(), 3, device=DEV), torch.randn(8, 3, device=DEV)
    out, saved, sarg = _C.spmm_pna_edge(g.csc, a, None, ef, w, PC.AGGS4, None, None, want_saved=True, eperm=_eperm(g))
    assert _C._lib.bot_last_kernel().decode() == "bot::spmm_pna_edge_kernel<4,4,8>"
    rec, _ = _C.pna_bwd_prep(g.csc, torch.randn(out.shape, device=DEV), PC.AGGS4, saved, sarg)
    _C.spmm_pna_edge_bwd(g.csr, g.csr2csc, a, ef, w, rec, PC.AGGS4, eperm=g.csr.eid, want_dweight=False)
    assert _C._lib.bot_last_kernel().decode() == "bot::spmm_pna_edge_bwd_kernel<dx,4,4,8>"
    _C.spmm_pna_edge_bwd(g.csr, g.csr2csc, a, ef, w, rec, PC.AGGS4, eperm=g.csr.eid, want_dx=False)
    assert _C._lib.bot_last_kernel().decode() == "bot::spmm_pna_edge_bwd_kernel<dw,4,4,8>"
    a16 = torch.randn(g.number_of_src_nodes(), 1000, device=DEV)
    ef16, w16 = torch.randn(g.number_of_edges(), 16, device=DEV), torch.randn(1000, 16, device=DEV)
    _C.spmm_pna_edge(g.csc, a16, None, ef16, w16, ("mean",), None, None, eperm=_eperm(g))
    assert _C._lib.bot_last_kernel().decode() == "bot::spmm_pna_edge_kernel<16,4,64>"        # tiles of 64 lanes


# ------------------------------------------------------------------------------------------------ 2. constant ef within every row
def _row_constant_ef(g, K, rng):
    """ef (edge-id order) whose rows are equal within every destination's in-edges."""
    indptr, _ = SG.csc_of(g)
    per_row = rng.standard_normal((g.number_of_dst_nodes(), K)).astype(np.float32)
    ef_pos = per_row[np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))]
    ef = np.zeros_like(ef_pos)
    ef[PE.position_rows(g)] = ef_pos
    return ef


@pytest.mark.parametrize("F_", (5, 64, 65, 256, 1000))
def test_constant_ef_within_a_row_gives_the_edge_less_moments_bytes(F_):
    """c_k - p_c = 0 for every k: S1 and S2 are the edge-less sweep's bit for bit, so var, std and the gate column are its bytes,
    whatever the weight."""
    aggs = ("var", "std")
    for name, g in _graphs()[2:] + (("sampled", _block()),):
        rng = np.random.default_rng(F_ + len(name))
        a = rng.standard_normal((g.number_of_src_nodes(), F_)).astype(np.float32)
        for K in _ks(F_)[:2]:
            ef, w = _dev(_row_constant_ef(g, K, rng)), _dev(rng.standard_normal((F_, K)).astype(np.float32))
            o, s, _ = _forward(g, a, None, ef, w, aggs, _ones(g), F_)
            o0, s0, _ = _C.spmm_pna(g.csc, _dev(a), None, aggs, _ones(g), F_, want_saved=True)
            assert _same_bytes(o, o0) and _same_bytes(s[:, F_:], s0[:, F_:]), (name, F_, K)


# ------------------------------------------------------------------------------------------------ 3. the exact regime
def _check_exact(g, F_, K, seed, pads=(0, 3, 4), tag="", dmax=8):
    """Tie values, small-integer ef, weight and b, integer dout: out, both position arrays, da, db and dweight entry for entry."""
    indptr, indices = SG.csc_of(g)
    n, n_src, E = g.number_of_dst_nodes(), g.number_of_src_nodes(), g.number_of_edges()
    rng = np.random.default_rng(seed)
    a = SG.tie_values(n_src, F_, seed)
    ef = rng.integers(-2, 3, (E, K)).astype(np.float32)
    w = rng.integers(-1, 2, (F_, K)).astype(np.float32)
    b = rng.integers(-3, 4, (n, F_)).astype(np.float32)
    ef_pos = ef[PE.position_rows(g)]
    vals, (amax, amin), info = PE.aggregate(indptr, indices, a, ef_pos, w, b)
    assert float(info["asum"].max()) + float(info["deg"].max()) * 3 < 2.0 ** 24
    want = PC.layout(np.stack([vals[k] for k in EXACT]), np.ones((1, n)), F_)
    dout = rng.integers(-dmax, dmax + 1, (n, 3 * F_)).astype(np.float32)
    da64, db64, dw64 = PE.exact_backward(indptr, indices, a, ef_pos, w, EXACT, dout, amax, amin)
    efd, wd, dd = _dev(ef), _dev(w), _dev(dout)
    for pad in pads:
        o, s, p = _forward(g, a, b, efd, wd, EXACT, _ones(g), F_, pad)
        assert np.array_equal(o.cpu().numpy().astype(np.float64), want), (tag, F_, K, pad)
        pn = p.cpu().numpy()
        assert np.array_equal(pn[:, :F_], amax) and np.array_equal(pn[:, F_:], amin), (tag, F_, K, pad)
        ad = _slab(a, pad)
        da, db, dw = _backward(g, ad, efd, wd, EXACT, dd, s, p, None, F_, pad)
        assert np.array_equal(da.cpu().double().numpy(), da64) and np.array_equal(db.cpu().double().numpy(), db64), (tag, F_, K, pad)
        assert np.array_equal(dw.cpu().double().numpy(), dw64), (tag, F_, K, pad)
        da2, _, dw2 = _backward(g, ad, efd, wd, EXACT, dd, s, p, None, F_)
        assert _same_bytes(da2, da) and _same_bytes(dw2, dw)


@pytest.mark.parametrize("F_", WIDTHS)
def test_forward_and_backward_are_exact_on_small_integers(F_):
    for name, g in _graphs():
        for K in _ks(F_):
            _check_exact(g, F_, K, 3 * F_ + K + len(name), pads=(0, 3, 4) if K == _ks(F_)[0] else (0,), tag=name)


@pytest.mark.parametrize("K", (3, 8))
@pytest.mark.parametrize("where", ("hub", "sampled"))
def test_exact_on_the_hub_graph_and_the_block(where, K):
    g = _hub()[0] if where == "hub" else _block()
    assert (_eperm(g) is None) == (where == "sampled")
    _check_exact(g, 40 if where == "sampled" else 8, K, 5, pads=(0,), tag=where, dmax=8 if where == "sampled" else 2)    # (dweight sums over 1e6 edges)


# ------------------------------------------------------------------------------------------------ 4. rounding bounds
RATIOS = {}


def _check_bounds(g, a, b, ef, w, Ft, tag):
    indptr, indices = SG.csc_of(g)
    n, F_, K = g.number_of_dst_nodes(), a.shape[1], ef.shape[1]
    ref, _, info = PE.aggregate(indptr, indices, a, ef[PE.position_rows(g)], w, b)
    o, s, p = _forward(g, a, b, _dev(ef), _dev(w), ALL6, _ones(g), Ft)
    o, s, p = o.cpu().numpy(), s.cpu().numpy(), p.cpu().numpy()
    SG.check_arg(indptr, p)
    T = F_ // Ft
    got = {k: o.astype(np.float64).reshape(n, T, 6, Ft)[:, :, i, :].reshape(n, F_) for i, k in enumerate(ALL6)}
    bound = PE.bounds(info, K)
    deg = info["deg"][:, None]
    err = {k: np.abs(got[k] - ref[k]) for k in ALL6}
    err["std"] = np.abs(got["std"] ** 2 - 1e-30 - ref["var"]) * (deg > 0)
    lim = {"mean": bound["mean"], "sum": bound["sum"], "var": bound["var"], "std": bound["var"] + 4 * U * got["std"] ** 2,
           "max": bound["ext"], "min": bound["ext"]}
    for k in ALL6:
        ratio = float((err[k] / np.maximum(lim[k], 1e-300)).max())
        RATIOS[k] = max(RATIOS.get(k, 0.0), ratio)
        print(f"{tag} Ft={Ft} {k}: worst error / bound = {ratio:.3f} (so far {RATIOS[k]:.3f})")
    for k in ALL6:
        assert bool((err[k] <= lim[k]).all()), (tag, k)
    some = (deg > 0) & np.ones((1, F_), dtype=bool)
    assert bool((s[~some[:, 0]] == 0).all()) and bool((o[~some[:, 0]] == 0).all()) and bool((p[~some[:, 0]] == -1).all())
    # a row of one neighbour has variance exactly 0, and the gate of the backward says so
    one = info["deg"] == 1
    assert one.any() or n < 3 or tag.startswith(("sampled", "hub"))         # (their rows all have several neighbours)
    assert bool((got["var"][one] == 0).all()) and bool((s[:, F_:][one] == 0).all())


@pytest.mark.parametrize("F_", (5, 64, 65, 256, 1000))     # 65: scalar lanes of a wide group; 1000: the walk over feature tiles
@pytest.mark.parametrize("shift", (0.0, 1000.0))
@pytest.mark.parametrize("ef_scale", (1.0, 30.0))
def test_forward_inside_the_rounding_bounds_shifted_or_not(F_, shift, ef_scale):
    """Seeded normal inputs; a and a + 1000 pass the SAME bounds (the split pivot's point), with ef of scale 1 and 30; the second K
    runs with ef constant within every row (where the moments are the edge-less sweep's)."""
    for name, g in _graphs()[2:] + (("sampled", _block()),):
        rng = np.random.default_rng(F_ + len(name))
        a = (rng.standard_normal((g.number_of_src_nodes(), F_)) + shift).astype(np.float32)
        b = rng.standard_normal((g.number_of_dst_nodes(), F_)).astype(np.float32)
        Ka, Kb = _ks(F_)[:2]
        ef = (ef_scale * rng.standard_normal((g.number_of_edges(), Ka))).astype(np.float32)
        w = rng.standard_normal((F_, Ka)).astype(np.float32)
        for Ft in _towers(F_)[:2]:
            _check_bounds(g, a, b, ef, w, Ft, f"{name} F={F_} K={Ka} shift={shift} ef x{ef_scale}")
        efc = (ef_scale * _row_constant_ef(g, Kb, rng)).astype(np.float32)
        _check_bounds(g, a, None, efc, rng.standard_normal((F_, Kb)).astype(np.float32), F_,
                      f"{name} F={F_} K={Kb} shift={shift} row-constant ef x{ef_scale} no b")


def test_bounds_on_the_hub_graph():
    g = _hub()[0]
    rng = np.random.default_rng(3)
    a = (rng.standard_normal((g.number_of_src_nodes(), 40)) + 1000.0).astype(np.float32)
    b = rng.standard_normal((g.number_of_dst_nodes(), 40)).astype(np.float32)
    ef = rng.standard_normal((g.number_of_edges(), 8)).astype(np.float32)
    _check_bounds(g, a, b, ef, rng.standard_normal((40, 8)).astype(np.float32), 40, "hub shift=1000")


# ------------------------------------------------------------------------------------------------ 5. backward on seeded normal inputs
def _op_against_autograd(g, F_, K, Ft, impl="kernel", seed=0, ef_grad=False):
    """ops.pna_aggregate_edge (4 aggregators x 3 scalers) forward + backward against float64 autograd of the restatement evaluated at
    the op's own owner positions."""
    indptr, indices = SG.csc_of(g)
    gen = torch.Generator().manual_seed(seed)
    a = torch.randn(g.number_of_src_nodes(), F_, generator=gen).to(DEV).requires_grad_()
    b = torch.randn(g.number_of_dst_nodes(), F_, generator=gen).to(DEV).requires_grad_()
    ef = torch.randn(g.number_of_edges(), K, generator=gen).to(DEV).requires_grad_(ef_grad)
    w = torch.randn(F_, K, generator=gen).to(DEV).requires_grad_()
    out, saved, sarg = ops.pna_aggregate_edge(g, a, b, ef, w, delta=1.6, tower_width=Ft, impl=impl, return_saved=True)
    assert not saved.requires_grad and sarg.dtype == torch.int32
    sg = sarg.cpu().numpy()
    SG.check_arg(indptr, sg)
    dout = torch.randn(out.shape, generator=gen)
    out.backward(dout.to(DEV))
    a64, b64, e64, w64 = (t.detach().cpu().double().requires_grad_() for t in (a, b, ef, w))
    rows = torch.from_numpy(PE.position_rows(g))
    ref = PE.pna_edge_torch(indptr, indices, a64, b64, e64[rows], w64, PC.AGGS4, PC.SCALERS3, 1.6, Ft, sg[:, :F_], sg[:, F_:])
    ref.backward(dout.double())
    fwd_close(out, ref.detach().numpy())
    grad_close(a.grad, a64.grad.numpy())
    grad_close(b.grad, b64.grad.numpy())
    grad_close(w.grad, w64.grad.numpy())
    if ef_grad:
        grad_close(ef.grad, e64.grad.numpy())
    return out.detach(), a.grad, b.grad, w.grad


def _grad_close_plus(got, want, term, tag):
    """`grad_close`'s criterion with a derived per-entry term: |got - want| <= GRAD_RTOL max|want| + term, every entry checked."""
    from tests.parity_cases import GRAD_RTOL
    got, want = got.detach().cpu().double().numpy(), np.asarray(want, dtype=np.float64)
    lim = GRAD_RTOL * float(np.abs(want).max()) + term
    err = np.abs(got - want)
    print(f"{tag}: worst error / criterion = {float((err / lim).max()):.3f}; entries whose derived term exceeds the suite's: "
          f"{int((term > GRAD_RTOL * float(np.abs(want).max())).sum())} of {term.size}, unbounded {int(np.isinf(term).sum())}")
    assert got.shape == want.shape and bool((err <= lim).all()), (tag, float((err / lim).max()))
    assert float(np.isinf(term).mean()) < 1e-3 and float((term > GRAD_RTOL * np.abs(want).max()).mean()) < 0.02, tag


@pytest.mark.parametrize("F_", WIDTHS)
def test_backward_against_fp64_autograd(F_):
    """da, db and dweight of all six aggregators x three scalers on seeded normal inputs against float64 autograd at the kernel's own
    owners; each gradient asked for alone gives the bytes it has beside the other; two calls give the same bytes.

    db is held to `grad_close` as it is.  da and dweight are held, EVERY entry, to `grad_close`'s criterion plus a per-entry term
    derived from the contract's order (tests/pna_edge_cases.py `std_gradient_terms`): std's gradient G (m_k - mean) / (n std) takes
    the float32 rounding of m_k - mean, at most (K + 4) u (|a_k| + C_k + |mean|), and the relative error of the forward's std, at
    most [3 u D + 2 K u max C + (deg + 4) u Dm^2 / std + 2 u std] / std.  On rows of ordinary spread the term is a few u of the
    gradient (it exceeds the suite's 1e-4 of the largest entry at fewer than 2 % of the entries, asserted); it grows where a row's
    messages lie together - a row of two neighbours whose a and c differ by 3 each and whose messages differ by 5e-5 has std 2.6e-5
    from deviations rounded at the ulp of 3, and the kernel's std there is off by 9e-4 of itself (measured: the one entry of all
    these cases, 0.0078 on a gradient of largest entry 33, that misses the bare criterion).  That is the split pivot's price, not an
    error of the order: the single pivot would round at the ulp of the messages instead.  The worst ratio is printed per case."""
    for name, g in _graphs()[3:] + (("sampled", _block()),):
        indptr, indices = SG.csc_of(g)
        rng = np.random.default_rng(11 * F_ + len(name))
        scale = ops.pna_scale_table(g, PC.SCALERS3, 1.6)
        rows = torch.from_numpy(PE.position_rows(g))
        for K in _ks(F_)[:2]:
            a = rng.standard_normal((g.number_of_src_nodes(), F_)).astype(np.float32)
            b = rng.standard_normal((g.number_of_dst_nodes(), F_)).astype(np.float32)
            ef = rng.standard_normal((g.number_of_edges(), K)).astype(np.float32)
            w = rng.standard_normal((F_, K)).astype(np.float32)
            Ft = _towers(F_)[-1]
            efd, wd = _dev(ef), _dev(w)
            o, s, p = _forward(g, a, b, efd, wd, ALL6, scale, Ft)
            dout = torch.randn(o.shape, generator=torch.Generator().manual_seed(K))
            ad = _dev(a)
            da, db, dw = _backward(g, ad, efd, wd, ALL6, dout.to(DEV), s, p, scale, Ft)
            sg = p.cpu().numpy()
            a64, b64, e64, w64 = (torch.from_numpy(t).double().requires_grad_() for t in (a, b, ef, w))
            PE.pna_edge_torch(indptr, indices, a64, b64, e64[rows], w64, ALL6, PC.SCALERS3, 1.6, Ft, sg[:, :F_], sg[:, F_:]).backward(dout.double())
            term_da, term_dw = PE.std_gradient_terms(indptr, indices, a, ef[rows.numpy()], w, ALL6, PC.SCALERS3, 1.6, Ft, dout.numpy())
            _grad_close_plus(da, a64.grad.numpy(), term_da, f"{name} F={F_} K={K} da")
            grad_close(db, b64.grad.numpy())
            _grad_close_plus(dw, w64.grad.numpy(), term_dw, f"{name} F={F_} K={K} dweight")
            da1, _, none = _backward(g, ad, efd, wd, ALL6, dout.to(DEV), s, p, scale, Ft, want_dweight=False)
            none2, _, dw1 = _backward(g, ad, efd, wd, ALL6, dout.to(DEV), s, p, scale, Ft, want_dx=False)
            assert none is None and none2 is None and _same_bytes(da1, da) and _same_bytes(dw1, dw), (name, F_, K)
            da2, db2, dw2 = _backward(g, ad, efd, wd, ALL6, dout.to(DEV), s, p, scale, Ft)
            assert _same_bytes(da2, da) and _same_bytes(db2, db) and _same_bytes(dw2, dw), (name, F_, K)


def test_backward_at_k16_on_a_large_graph_unmasked():
    """The KP = 16 instance (one staged neighbour per step) on a graph of 4 000 nodes at F = 64, std among the aggregators, by the bare
    `grad_close` through the op."""
    _op_against_autograd(_parent(), 64, 16, 16, seed=6)


def test_backward_on_the_hub_graph():
    _op_against_autograd(_hub()[0], 40, 8, 20, seed=4)


# ------------------------------------------------------------------------------------------------ 6. NaN and +-inf
def test_nan_and_inf_stay_inside_their_rows_and_columns():
    name, g = _graphs()[4]
    indptr, indices = SG.csc_of(g)
    n, F_, K = g.number_of_dst_nodes(), 12, 3
    rng = np.random.default_rng(2)
    a = rng.standard_normal((g.number_of_src_nodes(), F_)).astype(np.float32)
    ef = rng.standard_normal((g.number_of_edges(), K)).astype(np.float32)
    w = _dev(rng.standard_normal((F_, K)).astype(np.float32))
    clean = [t.clone() for t in _forward(g, a, None, _dev(ef), w, ALL6, _ones(g), F_)]
    # ef: every third destination's in-edges carry a NaN, +inf or -inf somewhere; the other rows keep their bytes
    seg = np.repeat(np.arange(n), np.diff(indptr))
    hit_rows = (np.arange(n) % 3 == 0) & (np.diff(indptr) > 0)
    ef_pos = ef[PE.position_rows(g)].copy()
    bad = np.array([np.nan, np.inf, -np.inf], dtype=np.float32)
    for k in np.nonzero(hit_rows[seg])[0][::2]:
        ef_pos[k, k % K] = bad[k % 3]
    ef_bad = np.zeros_like(ef)
    ef_bad[PE.position_rows(g)] = ef_pos
    o, s, p = _forward(g, a, None, _dev(ef_bad), w, ALL6, _ones(g), F_)
    torch.cuda.synchronize()
    SG.check_arg(indptr, p.cpu().numpy())
    keep = torch.from_numpy(~hit_rows).to(DEV)
    assert _same_bytes(o[keep], clean[0][keep]) and _same_bytes(s[keep], clean[1][keep]) and torch.equal(p[keep], clean[2][keep])
    assert not bool(torch.isfinite(o[~keep]).all())
    # a: NaN and +-inf in the even columns only; the odd columns keep their bytes
    a_bad = a.copy()
    a_bad[::3, ::2] = np.nan
    a_bad[1::3, ::2] = -np.inf
    a_bad[2::3, ::2] = np.inf
    o, s, p = _forward(g, a_bad, None, _dev(ef), w, ALL6, _ones(g), F_)
    torch.cuda.synchronize()
    SG.check_arg(indptr, p.cpu().numpy())
    odd = lambda t, width: t.reshape(n, -1, width)[:, :, 1::2]
    assert _same_bytes(odd(o, F_), odd(clean[0], F_)) and _same_bytes(odd(s, F_), odd(clean[1], F_))
    assert torch.equal(odd(p, F_), odd(clean[2], F_))
    # +-inf are ordinary values of a max and a min: with the NaNs taken out the extremes and their owners are the restatement's
    a_inf = np.where(np.isnan(a_bad), np.float32(0), a_bad)
    wi = np.random.default_rng(5).integers(-1, 2, (F_, K)).astype(np.float32)
    efi = np.random.default_rng(6).integers(-2, 3, ef.shape).astype(np.float32)
    o, s, p = _forward(g, a_inf, None, _dev(efi), _dev(wi), ("max", "min"), _ones(g), F_)
    vals, (amax, amin), _ = PE.aggregate(indptr, indices, a_inf, efi[PE.position_rows(g)], wi, None)
    on = o.cpu().numpy()
    assert np.array_equal(on[:, :F_], vals["max"].astype(np.float32)) and np.array_equal(on[:, F_:], vals["min"].astype(np.float32))
    assert np.array_equal(p.cpu().numpy()[:, :F_], amax) and np.array_equal(p.cpu().numpy()[:, F_:], amin)


# ------------------------------------------------------------------------------------------------ 7. routes
def test_routes_and_the_two_forms_agree(monkeypatch):
    name, g = _graphs()[6]
    calls = []
    real = _C.spmm_pna_edge
    monkeypatch.setattr(_C, "spmm_pna_edge", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    ok, dak, dbk, dwk = _op_against_autograd(g, 32, 8, 16, impl="kernel")
    assert len(calls) == 1
    ot, dat, dbt, dwt = _op_against_autograd(g, 32, 8, 16, impl="tensor")
    assert len(calls) == 1
    fwd_close(ok, ot.cpu().numpy())
    grad_close(dak, dat.cpu().numpy())
    grad_close(dbk, dbt.cpu().numpy())
    grad_close(dwk, dwt.cpu().numpy())
    _op_against_autograd(g, 32, 17, 16, impl="kernel")                 # K = 17: the tensor form
    assert len(calls) == 1
    _op_against_autograd(g, 32, 8, 16, impl="kernel", ef_grad=True)    # ef requires a gradient: the tensor form, and ef gets one
    assert len(calls) == 1
    _op_against_autograd(g, 32, 16, 16)                                # the default on the GPU
    assert len(calls) == (2 if ops.pna_edge_default_impl == "kernel" else 1)
    with torch.no_grad():                                              # no gradient is recorded: the kernel form whatever ef asks for
        gen = torch.Generator().manual_seed(0)
        a, ef, w = (torch.randn(s, generator=gen).to(DEV) for s in ((g.number_of_src_nodes(), 8), (g.number_of_edges(), 3), (8, 3)))
        before = len(calls)
        ops.pna_aggregate_edge(g, a, None, ef.requires_grad_(), w, impl="kernel")
        assert len(calls) == before + 1


# ------------------------------------------------------------------------------------------------ layers, stack, recipe
@pytest.mark.parametrize("shape", [(8, 8, 1, 3), (8, 8, 2, 3), (64, 64, 4, 8)])
@pytest.mark.parametrize("where", ["small", "block", "hub", "tensor"])
def test_edge_pnaconv_against_fp64_restatement(monkeypatch, shape, where):
    fin, fout, towers, K = shape
    if where == "small":
        PE.check_conv(_graphs()[3][1], DEV, monkeypatch, fin, fout, towers, K)             # isolated destinations
    elif where == "block":
        PE.check_conv(_block(), DEV, monkeypatch, fin, fout, towers, K, seed=1)
    elif where == "hub":
        PE.check_conv(_hub()[0], DEV, monkeypatch, fin, fout, towers, K, seed=2)
    else:
        PE.check_conv(_parent(), DEV, monkeypatch, fin, fout, towers, K, impl="tensor", seed=3)


def test_edge_pna_stack_against_fp64_restatement(monkeypatch):
    g = _parent()
    ef = torch.rand(g.number_of_edges(), 4, generator=torch.Generator().manual_seed(2))
    torch.manual_seed(3)
    model = bnn.EdgePNA(8, 5, 12, 3, edge_dim=4, delta=bnn.pna_delta(g), num_towers=2, dropout=0.5)
    PE.check_stack(model, g, g.ndata["feat"].cpu(), ef, DEV, monkeypatch)
    g.edata["feat"] = ef.to(DEV)
    try:
        nids = torch.randperm(g.number_of_nodes(), generator=torch.Generator().manual_seed(3))[:600]
        _, _, blocks = next(iter(NodeDataLoader(g, nids, MultiLayerNeighborSampler([5, 7, 9]), batch_size=600, seed=4)))
        per_block = [b.edata["feat"].cpu() for b in blocks]
        model2 = bnn.EdgePNA(8, 5, 12, 3, edge_dim=4, delta=1.5)
        PE.check_stack(model2, blocks, blocks[0].srcdata["feat"].cpu(), per_block, DEV, monkeypatch)
    finally:
        del g.edata["feat"]


def test_build_pna_edge_full_batch_step():
    wl = workloads.build_pna_edge("proteins", DEV, scale=0.002)
    loss, pred = wl.step()
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(pred).all())
    assert "spmm_pna_edge" in " ".join(k[0] for k in [wl.dominant])
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in wl.model.parameters())


def test_build_pna_edge_sampled_epoch():
    wl = workloads.build_pna_edge("proteins", DEV, sampled=True, scale=0.002)
    assert len(wl.loader) == workloads.SAMPLED["proteins"][1]
    loss = wl.epoch()
    assert np.isfinite(float(loss))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in wl.model.parameters())
