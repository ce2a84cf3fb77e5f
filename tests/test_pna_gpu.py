"""PNA on the MI355X: the fused multi-aggregator sweep, its backward pair (csrc/spmm_pna.hip) and `ops.pna_aggregate` against the float64
restatement (tests/pna_cases.py) - exactly where the arithmetic is exact (max, min, their owner positions, sums of small integers),
inside rounding bounds derived from the kernel's own summation order otherwise - `nn.PNAConv` and `nn.PNA` against their float64
restatements under the suite's criteria (tests/parity_cases.py), `fn.min`, and one train step / one sampled epoch of
`workloads.build_pna`.

The rounding bounds (u = 2^-24, deg = the row's in-degree, d_k = a_k - p with p the row's first neighbour, all from the restatement):
    mean   (deg + 2) u (max|d| + |p| + |b|)
    sum    (deg + 2) u sum_k (|a_k| + |b|)        - the messages are a_k + b; without b this is the issue's sum_k |a_k|
    var    (3 deg + 8) u max_k d_k^2; std is compared as out^2 - 1e-30 against var, plus 4 u out^2 for the root and the square
They are bounds for position-order sums; the chunks of a long row are summed chunk by chunk and then in slot order, a blocked form of the
same order whose error the same bound covers.  The SAME bounds hold for a + 1000: this is what a raw-moment kernel fails
(tests/test_pna_host.py shows the raw formula failing them in float32 on the CPU)."""
import numpy as np
import pytest
import torch

import bot_amd
from bot_amd import _C, ops, workloads
from bot_amd import function as fn
from bot_amd import nn as bnn
from bot_amd.sampling import MultiLayerNeighborSampler, NodeDataLoader
from tests import pna_cases as PC
from tests import sage_cases as SG
from tests.parity_cases import fwd_close, grad_close
from tests.test_sage_gpu import _block, _graphs, _hub, _parent, _same_bytes, _slab

pytestmark = pytest.mark.gpu
DEV = "cuda"
WIDTHS = (1, 3, 4, 5, 40, 64, 65, 256, 1000)     # every lane width and group size; 1000 walks feature tiles
EXACT = ("sum", "max", "min")
ALL6 = ("mean", "sum", "max", "min", "std", "var")
U = PC.U32


def _towers(F_):
    return [F_ // t for t in (1, 2, 4) if F_ % t == 0]


def _ones(g):
    return torch.ones((1, g.number_of_dst_nodes()), device=DEV)


def _int_b(n, F_, seed):
    return np.random.default_rng(seed).integers(-3, 4, (n, F_)).astype(np.float32)


def _launch(g, a, b, aggs, scale, Ft, pad):
    """One `_C.spmm_pna` call on operands inside buffers `pad` columns wider than their rows -> (out, saved, sarg) as numpy, after the
    check that nothing was written beyond a row."""
    n, F_ = g.number_of_dst_nodes(), a.shape[1]
    W = scale.shape[0] * len(aggs) * F_
    ad, bd = _slab(a, pad), None if b is None else _slab(b, pad)
    out = torch.full((n, W + pad), 9.0, device=DEV)[:, :W] if pad else None
    saved = torch.full((n, 2 * F_ + pad), 9.0, device=DEV)[:, :2 * F_] if pad else None
    sarg = torch.full((n, 2 * F_ + pad), 9, dtype=torch.int32, device=DEV)[:, :2 * F_] if pad else None
    o, s, p = _C.spmm_pna(g.csc, ad, bd, aggs, scale, Ft, want_saved=True, out=out, saved=saved, sarg=sarg)
    if pad:
        assert o.data_ptr() == out.data_ptr() and s.data_ptr() == saved.data_ptr() and p.data_ptr() == sarg.data_ptr()
        assert bool((o._base[:, W:] == 9.0).all()) and bool((s._base[:, 2 * F_:] == 9.0).all()) and bool((p._base[:, 2 * F_:] == 9).all())
    o2, s2, p2 = _C.spmm_pna(g.csc, ad, bd, aggs, scale, Ft, want_saved=True)
    assert _same_bytes(o2, o) and _same_bytes(s2, s) and torch.equal(p2, p)
    return o.cpu().numpy(), s.cpu().numpy(), p.cpu().numpy()


def _check_exact(g, F_, seed, pads=(0, 3, 4), tag=""):
    """Tie values and small-integer b: sum, max, min and both position arrays entry for entry, every pad, tower width and b on / off."""
    indptr, indices = SG.csc_of(g)
    n = g.number_of_dst_nodes()
    a = SG.tie_values(g.number_of_src_nodes(), F_, seed)
    for b in (_int_b(n, F_, seed + 1), None):
        chosen, _, _ = PC.aggregate(indptr, indices, a, b, EXACT)
        vals = np.stack([chosen[k] for k in EXACT])
        amax, amin = PC.owners(indptr, indices, a)
        for pad in pads:
            for Ft in _towers(F_):
                want = PC.layout(vals, np.ones((1, n)), Ft)
                o, s, p = _launch(g, a, b, EXACT, _ones(g), Ft, pad)
                assert np.array_equal(o.astype(np.float64), want), (tag, F_, pad, Ft, b is None)
                assert np.array_equal(p[:, :F_], amax) and np.array_equal(p[:, F_:], amin), (tag, F_, pad, Ft)


# ------------------------------------------------------------------------------------------------ 1. forward, exact
@pytest.mark.parametrize("F_", WIDTHS)
def test_pna_forward_is_exact_on_tie_values(F_):
    for name, g in _graphs():
        _check_exact(g, F_, 3 * F_ + len(name), tag=name)
    assert "spmm_pna_kernel" in _C._lib.bot_last_kernel().decode()


def test_pna_forward_on_the_hub_graph_is_exact():
    g = _hub()[0]
    _check_exact(g, 40, 5, pads=(0,), tag="hub")


def test_pna_forward_with_nan_and_inf_stays_inside_the_row():
    name, g = _graphs()[4]
    indptr, indices = SG.csc_of(g)
    a = SG.tie_values(g.number_of_src_nodes(), 12, 1)
    a[::3, ::2] = np.nan
    a[1::3, 1::2] = -np.inf
    a[2::3, 1::2] = np.inf
    o, s, p = _C.spmm_pna(g.csc, torch.from_numpy(a).to(DEV), None, ALL6, _ones(g), None, want_saved=True)
    torch.cuda.synchronize()
    SG.check_arg(indptr, p.cpu().numpy())
    clean = np.where(np.isnan(a), np.float32(0), a)                    # +-inf are ordinary values of a max and a min
    o, s, p = _C.spmm_pna(g.csc, torch.from_numpy(clean).to(DEV), None, ("max", "min"), _ones(g), None, want_saved=True)
    chosen, _, _ = PC.aggregate(indptr, indices, clean, None, ("max", "min"))
    amax, amin = PC.owners(indptr, indices, clean)
    assert np.array_equal(o.cpu().numpy()[:, :12], chosen["max"].astype(np.float32)) and np.array_equal(o.cpu().numpy()[:, 12:], chosen["min"].astype(np.float32))
    assert np.array_equal(p.cpu().numpy()[:, :12], amax) and np.array_equal(p.cpu().numpy()[:, 12:], amin)


# ------------------------------------------------------------------------------------------------ 2. forward, rounding bounds
def _check_bounds(g, a, b, Ft, tag):
    indptr, indices = SG.csc_of(g)
    n, F_ = g.number_of_dst_nodes(), a.shape[1]
    _, ref, info = PC.aggregate(indptr, indices, a, b, ALL6)
    o, s, p = _launch(g, a, b, ALL6, _ones(g), Ft, 0)
    T = F_ // Ft
    got = {k: o.astype(np.float64).reshape(n, T, 6, Ft)[:, :, i, :].reshape(n, F_) for i, k in enumerate(ALL6)}
    deg = info["deg"][:, None].astype(np.float64)
    err = {k: np.abs(got[k] - ref[k]) for k in ALL6}
    bound = {"mean": (deg + 2) * U * (info["dmax"] + np.abs(info["p"]) + info["babs"]),
             "sum": (deg + 2) * U * (info["asum"] + deg * info["babs"]),
             "var": (3 * deg + 8) * U * info["dmax"] ** 2}
    for k in ("mean", "sum", "var"):
        print(f"{tag} Ft={Ft} {k}: worst error / bound = {float((err[k] / np.maximum(bound[k], 1e-300)).max()):.3f}")
    std_err = np.abs(got["std"] ** 2 - 1e-30 - ref["var"]) * (deg > 0)
    print(f"{tag} Ft={Ft} std: worst error / bound = {float((std_err / np.maximum(bound['var'] + 4 * U * got['std'] ** 2, 1e-300)).max()):.3f}")
    for k in ("mean", "sum", "var"):
        assert bool((err[k] <= bound[k]).all()), (tag, k)
    assert bool((std_err <= bound["var"] + 4 * U * got["std"] ** 2).all()), tag
    some = (deg > 0) & np.ones((1, F_), dtype=bool)
    assert bool((err["max"] <= 2 * U * np.abs(ref["max"])).all()) and bool((err["min"] <= 2 * U * np.abs(ref["min"])).all())   # one add of b
    assert bool((s[:, :F_][~some] == 0).all()) and bool((o[~some[:, 0]] == 0).all())
    # a row of one neighbour has variance exactly 0, and the gate of the backward says so
    one = info["deg"] == 1
    assert one.any() or n < 3
    assert bool((got["var"][one] == 0).all()) and bool((s[:, F_:][one] == 0).all())


@pytest.mark.parametrize("F_", (5, 40, 64, 256))
@pytest.mark.parametrize("shift", (0.0, 1000.0))
def test_pna_forward_inside_the_rounding_bounds_shifted_or_not(F_, shift):
    """The shifted case passes the SAME bounds as the unshifted one (the pivot's point)."""
    for name, g in _graphs()[2:]:
        rng = np.random.default_rng(F_ + len(name))
        a = (rng.standard_normal((g.number_of_src_nodes(), F_)) + shift).astype(np.float32)
        b = rng.standard_normal((g.number_of_dst_nodes(), F_)).astype(np.float32)
        for Ft in _towers(F_)[:2]:
            _check_bounds(g, a, b, Ft, f"{name} F={F_} shift={shift}")
        _check_bounds(g, a, None, F_, f"{name} F={F_} shift={shift} no b")


def test_pna_scalers_towers_and_the_constant_row_pivot():
    """4 aggregators x 3 scalers in every tower layout against the restatement, by the forward criterion.  With the pivot pointed at
    a's row 0 (what tools/bench_pna.py prices the pivot against) mean, max, min and var come out the same up to rounding; std is left
    out of that comparison: where a row's neighbours are equal only the neighbour pivot gives var = 0 exactly, and the root of a
    rounding error of 1e-7 is 3e-4."""
    name, g = _graphs()[6]
    indptr, indices = SG.csc_of(g)
    rng = np.random.default_rng(4)
    a = rng.standard_normal((g.number_of_src_nodes(), 64)).astype(np.float32)
    b = rng.standard_normal((g.number_of_dst_nodes(), 64)).astype(np.float32)
    scale = ops.pna_scale_table(g, PC.SCALERS3, 1.9)
    np.testing.assert_allclose(scale.cpu().numpy(), PC.scale_table(indptr, PC.SCALERS3, 1.9), rtol=1e-6, atol=0)
    no_std = ("mean", "max", "min", "var")
    for Ft in (64, 32, 16):
        want, _ = PC.pna_forward(indptr, indices, a, b, PC.AGGS4, PC.SCALERS3, 1.9, Ft)
        o, _, _ = _launch(g, a, b, PC.AGGS4, scale, Ft, 4)
        fwd_close(torch.from_numpy(o), want)
        want0, _ = PC.pna_forward(indptr, indices, a, b, no_std, PC.SCALERS3, 1.9, Ft)
        o0, _, _ = _C.spmm_pna(g.csc, torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), no_std, scale, Ft, pivot=False)
        fwd_close(o0, want0)


# ------------------------------------------------------------------------------------------------ 3. backward
def _check_backward_exact(g, F_, seed, pads=(0, 3, 4), tag=""):
    """Tie values, integer dout in [-8, 8] (the mean block times the in-degree, so that its G / n is an integer): da and db of the
    mean, sum, max and min paths entry for entry against float64 autograd of the restatement, and every column's gradient mass."""
    aggs = ("mean", "sum", "max", "min")
    indptr, indices = SG.csc_of(g)
    n, n_src = g.number_of_dst_nodes(), g.number_of_src_nodes()
    rng = np.random.default_rng(seed)
    a = SG.tie_values(n_src, F_, seed)
    amax, amin = PC.owners(indptr, indices, a)
    deg = np.diff(indptr)[:, None]
    for Ft in _towers(F_):
        T = F_ // Ft
        dout = rng.integers(-8, 9, (n, T, 4, Ft)).astype(np.float32)
        dout[:, :, 0, :] *= deg[:, :, None]
        dout = dout.reshape(n, 4 * F_)
        a64 = torch.from_numpy(a).double().requires_grad_()
        b64 = torch.zeros((n, F_), dtype=torch.float64, requires_grad=True)
        PC.pna_torch(indptr, indices, a64, b64, aggs, ("identity",), 1.0, Ft, amax, amin).backward(torch.from_numpy(dout).double())
        saved = np.zeros((n, 2 * F_), dtype=np.float32)              # (these four paths read neither the mean nor the std)
        sarg = np.concatenate([amax, amin], axis=1)
        for pad in pads:
            dd, sv, sg, ad = _slab(dout, pad), _slab(saved, pad), _slab(sarg, pad), _slab(a, pad)
            R = _C.pna_record_sections(aggs) * F_
            rec = torch.full((n, R + pad), 9.0, device=DEV)[:, :R] if pad else None
            db = torch.full((n, F_ + pad), 9.0, device=DEV)[:, :F_] if pad else None
            dx = torch.full((n_src, F_ + pad), 9.0, device=DEV)[:, :F_] if pad else None
            rec, db = _C.pna_bwd_prep(g.csc, dd, aggs, sv, sg, None, Ft, rec=rec, db=db)
            da = _C.spmm_pna_bwd(g.csr, g.csr2csc, ad, rec, aggs, out=dx)
            assert np.array_equal(da.cpu().double().numpy(), a64.grad.numpy()), (tag, F_, Ft, pad)
            assert np.array_equal(db.cpu().double().numpy(), b64.grad.numpy()), (tag, F_, Ft, pad)
            assert np.array_equal(da.cpu().double().numpy().sum(0), db.cpu().double().numpy().sum(0))      # the mass of every column
            if pad:
                assert bool((rec._base[:, R:] == 9.0).all()) and bool((db._base[:, F_:] == 9.0).all()) and bool((da._base[:, F_:] == 9.0).all())
            rec2, db2 = _C.pna_bwd_prep(g.csc, dd, aggs, sv, sg, None, Ft)
            assert _same_bytes(rec2, rec) and _same_bytes(db2, db) and _same_bytes(_C.spmm_pna_bwd(g.csr, g.csr2csc, ad, rec2, aggs), da)


@pytest.mark.parametrize("F_", WIDTHS)
def test_pna_backward_is_exact_on_tie_values(F_):
    for name, g in _graphs():
        _check_backward_exact(g, F_, 5 * F_ + len(name), tag=name)
    assert "spmm_pna_bwd_kernel" in _C._lib.bot_last_kernel().decode()


def test_pna_backward_on_the_hub_graph_is_exact():
    _check_backward_exact(_hub()[0], 40, 17, pads=(0,), tag="hub")


def test_pna_sweeps_on_the_edge_case_graph_at_32_lanes():
    """The one group width WIDTHS leaves out (17 columns of 4-byte lanes: groups of 32), forward and backward, on SG.sweep_edges: with
    chunk = 8 its rows above 8 in-edges run as chunks of a long row, with chunk = 128 the rows of 63 / 64 / 65 in-edges are walked
    whole, 32 ids at a time."""
    src, dst, n = SG.sweep_edges()
    for chunk in (8, 128):
        g = bot_amd.Graph(src, dst, n, chunk=chunk).to(DEV)
        assert (g.csc.n_long > 0 and g.csr.n_long > 0) == (chunk == 8)
        _check_exact(g, 17, 23, pads=(0,), tag=f"chunk{chunk}")
        assert _C._lib.bot_last_kernel().decode() == "bot::spmm_pna_kernel<1,32,1>"
        _check_backward_exact(g, 17, 29, pads=(0,), tag=f"chunk{chunk}")
        assert _C._lib.bot_last_kernel().decode() == "bot::spmm_pna_bwd_kernel<1,32,1>"


def _op_against_autograd(g, a_np, b_np, Ft, impl="kernel", seed=0):
    """ops.pna_aggregate (4 aggregators x 3 scalers) forward + backward against float64 autograd of the restatement fed the op's own
    owner positions: the forward criterion, grad_close for da and db."""
    indptr, indices = SG.csc_of(g)
    F_ = a_np.shape[1]
    a = torch.from_numpy(a_np).to(DEV).requires_grad_()
    b = torch.from_numpy(b_np).to(DEV).requires_grad_()
    out, saved, sarg = ops.pna_aggregate(g, a, b, delta=1.6, tower_width=Ft, impl=impl, return_saved=True)
    assert not saved.requires_grad and sarg.dtype == torch.int32
    sg = sarg.cpu().numpy()
    SG.check_arg(indptr, sg)
    dout = torch.randn(out.shape, generator=torch.Generator().manual_seed(seed))
    out.backward(dout.to(DEV))
    a64, b64 = a.detach().cpu().double().requires_grad_(), b.detach().cpu().double().requires_grad_()
    ref = PC.pna_torch(indptr, indices, a64, b64, PC.AGGS4, PC.SCALERS3, 1.6, Ft, sg[:, :F_], sg[:, F_:])
    ref.backward(dout.double())
    fwd_close(out, ref.detach().numpy(), rtol=2e-6)       # (the shifted operands are of the size of 10: 1e-4 absolute + float32's own)
    grad_close(a.grad, a64.grad.numpy())
    grad_close(b.grad, b64.grad.numpy())
    return out.detach(), a.grad, b.grad


@pytest.mark.parametrize("F_", (5, 64, 256))
@pytest.mark.parametrize("shift", (0.0, 8.0))
def test_pna_backward_against_float64_autograd_shifted_or_not(F_, shift):
    for name, g in (_graphs()[3], _graphs()[5], _graphs()[6]):
        assert bool((g.in_degrees() == 1).any())                           # rows of one neighbour: the var == 0 gate is exercised
        rng = np.random.default_rng(F_ + len(name))
        a = (rng.standard_normal((g.number_of_src_nodes(), F_)) + shift).astype(np.float32)
        b = rng.standard_normal((g.number_of_dst_nodes(), F_)).astype(np.float32)
        for Ft in _towers(F_)[-2:]:
            o1, da1, db1 = _op_against_autograd(g, a, b, Ft)
            o2, da2, db2 = _op_against_autograd(g, a, b, Ft)
            assert _same_bytes(o1, o2) and _same_bytes(da1, da2) and _same_bytes(db1, db2)


def test_rows_of_one_neighbour_and_constant_rows_have_exactly_zero_std_gradient():
    name, g = _graphs()[5]
    indptr, indices = SG.csc_of(g)
    n, n_src, F_ = g.number_of_dst_nodes(), g.number_of_src_nodes(), 12
    deg = np.diff(indptr)
    rng = np.random.default_rng(2)
    a = (rng.standard_normal((n_src, F_)) + 3).astype(np.float32)
    const = int(np.nonzero(deg > 4)[0][0])
    a[indices[indptr[const]:indptr[const + 1]]] = a[indices[indptr[const]]]      # every neighbour of `const` holds the same row
    flat = (deg == 1)
    flat[const] = True
    for aggs in (("std",), ("var",), ("std", "var")):
        x = torch.from_numpy(a).to(DEV).requires_grad_()
        out, saved, _ = ops.pna_aggregate(g, x, None, aggs, ("identity", "amplification"), 1.2, return_saved=True)
        o = out.detach().cpu().numpy().reshape(n, 2, len(aggs), F_)
        for i, k in enumerate(aggs):
            if k == "var":
                assert bool((o[flat][:, 0, i] == 0).all())
            else:                                                          # sqrt(0 + 1e-30)
                np.testing.assert_allclose(o[flat][:, 0, i], 1e-15, rtol=1e-6, atol=0)
        assert bool((saved.cpu().numpy()[flat][:, F_:] == 0).all())
        dout = torch.zeros(out.shape)
        dout[torch.from_numpy(flat)] = torch.randn(int(flat.sum()), out.shape[1], generator=torch.Generator().manual_seed(1))
        out.backward(dout.to(DEV))
        assert bool((x.grad == 0).all())


# ------------------------------------------------------------------------------------------------ 4. op, reducer, layer, stack
def test_kernel_and_tensor_forms_agree():
    name, g = _graphs()[6]
    rng = np.random.default_rng(9)
    a = rng.standard_normal((g.number_of_src_nodes(), 32)).astype(np.float32)
    b = rng.standard_normal((g.number_of_dst_nodes(), 32)).astype(np.float32)
    ok, dak, dbk = _op_against_autograd(g, a, b, 16, impl="kernel")
    ot, dat, dbt = _op_against_autograd(g, a, b, 16, impl="tensor")
    fwd_close(ok, ot.cpu().numpy())
    grad_close(dak, dat.cpu().numpy())
    grad_close(dbk, dbt.cpu().numpy())
    with pytest.raises(ValueError, match="impl"):
        ops.pna_aggregate(g, torch.from_numpy(a).to(DEV), impl="triton")


def test_update_all_min_is_the_negated_max_of_the_negation():
    for name, g in (_graphs()[3], _graphs()[4]):
        n = g.number_of_nodes()
        for shape in ((6,), (41,), (3, 4)):
            x = torch.randn((n,) + shape, device=DEV)
            g.ndata["h"] = x
            g.update_all(fn.copy_u("h", "m"), fn.min("m", "o"))
            assert "spmm_pna_kernel" in _C._lib.bot_last_kernel().decode()
            want = -ops.copy_u_max(g, -x)
            some = g.in_degrees() > 0
            assert _same_bytes(g.ndata["o"][some], want[some]) and torch.equal(g.ndata["o"], want)      # (an empty row: 0.0, there -0.0)
            assert bool((g.ndata["o"][~some] == 0).all())
        x = torch.randn(n, 8, device=DEV, requires_grad=True)
        ops.copy_u_min(g, x).sum().backward()
        x2 = x.detach().clone().requires_grad_()
        (-ops.copy_u_max(g, -x2)).sum().backward()
        assert torch.equal(x.grad, x2.grad)
        g.edata["w"] = torch.rand(g.number_of_edges(), 1, device=DEV)
        with pytest.raises(NotImplementedError, match="min"):
            g.update_all(fn.u_mul_e("h", "w", "m"), fn.min("m", "o"))


def test_last_kernel_names_the_pna_kernels():
    name, g = _graphs()[4]                                             # long rows: the combine runs behind the sweep
    a = torch.randn(g.number_of_src_nodes(), 8, device=DEV)
    out, saved, sarg = _C.spmm_pna(g.csc, a, None, PC.AGGS4, None, None, want_saved=True)
    assert _C._lib.bot_last_kernel().decode() == "bot::spmm_pna_kernel<4,8,1>"
    rec, db = _C.pna_bwd_prep(g.csc, torch.randn(out.shape, device=DEV), PC.AGGS4, saved, sarg)
    assert _C._lib.bot_last_kernel().decode() == "bot::pna_bwd_prep_kernel"
    _C.spmm_pna_bwd(g.csr, g.csr2csc, a, rec, PC.AGGS4)
    assert _C._lib.bot_last_kernel().decode() == "bot::spmm_pna_bwd_kernel<4,8,1>"


@pytest.mark.parametrize("towers", (1, 2))
@pytest.mark.parametrize("residual", (True, False))
def test_pnaconv_against_fp64_restatement(monkeypatch, towers, residual):
    PC.check_conv(_parent(), DEV, monkeypatch, 16, 16, towers, residual)
    PC.check_conv(_block(), DEV, monkeypatch, 16, 24, towers, residual, seed=1)
    PC.check_conv(_graphs()[3][1], DEV, monkeypatch, 8, 8, towers, residual, seed=2)          # isolated destinations
    PC.check_conv(_parent(), DEV, monkeypatch, 16, 16, towers, residual, impl="tensor", seed=3)


def test_pna_stack_against_fp64_restatement(monkeypatch):
    g = _parent()
    torch.manual_seed(3)
    model = bnn.PNA(8, 5, 12, 3, delta=bnn.pna_delta(g), num_towers=2, dropout=0.5)
    PC.check_stack(model, g, g.ndata["feat"].cpu(), DEV, monkeypatch)
    nids = torch.randperm(g.number_of_nodes(), generator=torch.Generator().manual_seed(3))[:600]
    _, _, blocks = next(iter(NodeDataLoader(g, nids, MultiLayerNeighborSampler([5, 7, 9]), batch_size=600, seed=4)))
    model2 = bnn.PNA(8, 5, 12, 3, delta=1.5)
    PC.check_stack(model2, blocks, blocks[0].srcdata["feat"].cpu(), DEV, monkeypatch)


def test_build_pna_full_batch_step():
    wl = workloads.build_pna("cora", DEV, scale=0.25)
    res = wl.step()
    assert all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in res[3:6])
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in wl.model.parameters())


def test_build_pna_sampled_epoch():
    wl = workloads.build_pna("cora", DEV, sampled=True, scale=0.25)
    assert len(wl.loader) == workloads.SAMPLED["cora"][1]
    loss = wl.epoch()
    assert np.isfinite(float(loss))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in wl.model.parameters())
