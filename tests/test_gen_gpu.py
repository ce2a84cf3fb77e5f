"""DeeperGCN on the MI355X: the softmax-aggregation sweep pair (csrc/spmm_softmax.hip) entry for entry in its two exact regimes (beta = 0:
the float32 mean; beta = 128 over integers: the max sweep's bytes, and its backward), against the float64 restatement
(tests/gen_cases.py) under bounds derived from the row lengths and the measured error of the kernel's exponential, against the tensor
form, `nn.GENConv` / `nn.DeeperGCN` against their float64 restatements under the suite's own criteria, and one train step / one sampled
epoch of `workloads.build_gen`.

Measured on the MI355X (the figures the README section "DeeperGCN / softmax aggregation" carries): see `test_report_measured_figures`,
which prints the exponential's error and the largest error / bound ratios the module saw."""
import functools

import numpy as np
import pytest
import torch

import bot_amd
from bot_amd import _C, ops, workloads
from bot_amd import nn as bnn
from bot_amd.sampling import MultiLayerNeighborSampler, NodeDataLoader
from tests import gen_cases as GC
from tests import sage_cases as SG
from tests.parity_cases import grad_close
from tests.test_sage_gpu import _block, _graphs, _parent, _same_bytes, _slab

pytestmark = pytest.mark.gpu
DEV = "cuda"
WIDTHS = (1, 3, 4, 5, 40, 64, 65, 256, 1000)     # every lane width and group size; 1000 walks feature tiles
BETAS = (0.1, 1.0, 10.0)
EPS = 1e-7
RATIOS = {}                                        # name -> the largest |error| / bound seen by the toleranced tests


def _beta(v):
    return torch.full((1,), float(v), dtype=torch.float32, device=DEV)


def _ratio(name, err, tol):
    """Records max(err / tol) under `name` and returns the entries over their bound."""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))
    RATIOS[name] = max(RATIOS.get(name, 0.0), float(r.max()) if r.size else 0.0)
    return np.argwhere(err > tol)


@functools.lru_cache(maxsize=None)
def _simple_graphs():
    """The shapes of tests.test_sage_gpu._graphs() without parallel edges (a unique maximum per row and column exists)."""
    out = [(f"square{n}", GC.simple_graph(n, n, n).to(DEV)) for n in (1, 63, 64, 65)]
    out.append(("long65", GC.simple_graph(65, 65, 70, chunk=4).to(DEV)))
    out.append(("block", GC.simple_graph(63, 200, 71).to(DEV)))
    out.append(("longblock", GC.simple_graph(64, 130, 72, chunk=4).to(DEV)))
    assert out[4][1].csc.n_long > 0 and out[4][1].csr.n_long > 0
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _hub():
    from tests.test_subgraph_gpu import _hub_graph
    g = _hub_graph()
    indptr, indices = SG.csc_of(g)
    assert int(np.diff(indptr).max()) > 2048 and g.csc.n_long > 0 and g.csr.n_long > 0
    return g, indptr, indices


# ------------------------------------------------------------------------------------------------ 0. the kernel's exponential
@functools.lru_cache(maxsize=None)
def _exp_error():
    """The largest relative error of the kernel's exponential against float64, read back from a one-row graph: one source with one
    out-edge, x = out = 0, dout = 1, beta = 1 and lse = -t make the backward sweep store exp(t) itself (beta m - lse = t exactly,
    1 + beta (m - out) = 1, one term).  Relative error over t in [-87, 0], where exp(t) is a normal float32; below, down to -104, the
    instruction flushes to zero and the error is at most 2^-126 ABSOLUTE (asserted here; the bounds carry it as GC.TINY)."""
    g = bot_amd.Graph(torch.tensor([0]), torch.tensor([0]), 1, num_dst_nodes=1).to(DEV)
    F_ = 8192
    worst = literal = 0.0
    for seed in range(3):
        rng = np.random.default_rng(seed)
        t = (-104.0 * rng.random(F_)).astype(np.float32)
        t[:4] = [0.0, -87.0, -104.0, -1.0]
        t[4:4 + 1024] = np.linspace(-87.0, 0.0, 1024, dtype=np.float32)
        z = torch.zeros(1, F_, device=DEV)
        got = _C.spmm_softmax_bwd(g.csr, z, _beta(1.0), False, 0.0, torch.ones(1, F_, device=DEV), torch.zeros(1, F_, device=DEV),
                                  torch.from_numpy(-t).to(DEV).reshape(1, F_)).cpu().double().numpy()[0]
        want = np.exp(t.astype(np.float64))
        normal = t >= -87.0
        worst = max(worst, float((np.abs(got - want)[normal] / want[normal]).max()))
        literal = max(literal, float((np.abs(got - want) / want).max()))
        assert float(np.abs(got - want)[~normal].max()) <= GC.TINY
    assert got[0] == 1.0                           # exp(0) is exactly 1: what the beta = 0 regime rests on
    # taken literally over all of [-104, 0] the relative error is 1: below -87.34 the true value is a denormal, or below the smallest
    # one, and the stored 0 is off by all of it; a bound built on that figure would hold for any kernel, so it is printed, not used
    print(f"relative error of the kernel's exponential over all of [-104, 0], flushed results included: {literal:.3f}")
    return worst


def test_exponential_error_is_a_few_units_in_the_last_place():
    """Not a bound taken from the code under test: v_exp_f32 is specified to 1 ulp and the first-order correction adds two roundings, so
    anything above 4 * 2^-24 would be a finding."""
    e = _exp_error()
    print(f"measured: largest relative error of the kernel's exponential over [-87, 0] = {e:.3e} ({e / GC.U:.2f} U)")
    assert e <= 4 * GC.U


# ------------------------------------------------------------------------------------------------ 1. forward, exact regimes
def _ints(n, F_, seed):
    return np.random.default_rng(seed).integers(-8, 9, (n, F_)).astype(np.float32)


def _forward(g, xd, beta, relu, want_q, pad, eps=0.0):
    n, F_ = g.number_of_dst_nodes(), xd.shape[1]
    bufs = [torch.full((n, F_ + pad), 9.0, device=DEV)[:, :F_] if pad else None for _ in range(3)]
    o, l, q = _C.spmm_softmax(g.csc, xd, _beta(beta), relu, eps, want_q, out=bufs[0], lse=bufs[1], q=bufs[2] if want_q else None)
    if pad:
        assert o.data_ptr() == bufs[0].data_ptr() and l.data_ptr() == bufs[1].data_ptr()
        assert all(bool((t._base[:, F_:] == 9.0).all()) for t in (o, l) + ((q,) if want_q else ()))     # nothing beyond the row
    assert (q is not None) == want_q
    return o, l, q


def _check_exact_forward(name, g, F_, seed):
    indptr, indices = SG.csc_of(g)
    x = _ints(g.number_of_src_nodes(), F_, seed)
    for relu in (False, True):
        mean = GC.mean32(indptr, indices, x, relu)
        m = np.maximum(x, 0) if relu else x
        mean_sq = GC.mean32(indptr, indices, m * m, False)
        for pad in (0, 3, 4):                     # contiguous; an odd row stride (4-byte lanes); a strided slab that keeps wide lanes
            xd = _slab(x, pad)
            want_q = pad != 3
            # beta = 0: every weight is exactly 1
            o, l, q = _forward(g, xd, 0.0, relu, want_q, pad)
            assert _same_bytes(o, torch.from_numpy(mean).to(DEV)), (name, F_, relu, pad)
            if want_q:
                assert _same_bytes(q, torch.from_numpy(mean_sq).to(DEV)), (name, F_, relu, pad)
            o2, l2, q2 = _C.spmm_softmax(g.csc, xd, _beta(0.0), relu, 0.0, not want_q)
            assert _same_bytes(o2, o) and _same_bytes(l2, l)          # the same bytes again, with or without q
            # beta = 128: every exponent off the maximum underflows to 0
            mx, _ = _C.spmm_max(g.csc, xd, relu)
            o, l, q = _forward(g, xd, 128.0, relu, want_q, pad)
            assert _same_bytes(o, mx), (name, F_, relu, pad)
            if want_q:
                assert _same_bytes(q, mx * mx), (name, F_, relu, pad)
            o2, l2, _ = _C.spmm_softmax(g.csc, xd, _beta(128.0), relu, 0.0, want_q)
            assert _same_bytes(o2, o) and _same_bytes(l2, l)
    empty = torch.from_numpy(np.diff(indptr) == 0).to(DEV)
    assert bool((l[empty] == 0).all()) and bool((o[empty] == 0).all())


@pytest.mark.parametrize("F_", WIDTHS)
def test_forward_exact_regimes(F_):
    for name, g in _graphs():
        _check_exact_forward(name, g, F_, 3 * F_ + len(name))
    assert "spmm_softmax_kernel" in _C._lib.bot_last_kernel().decode()


def test_forward_exact_regimes_on_the_edge_case_graph_at_32_lanes():
    """The one group width WIDTHS leaves out (17 columns of 4-byte lanes: groups of 32) on SG.sweep_edges: with chunk = 8 its rows above
    8 in-edges run as chunks of a long row, with chunk = 128 the rows of 63 / 64 / 65 in-edges are walked whole."""
    src, dst, n = SG.sweep_edges()
    for chunk in (8, 128):
        g = bot_amd.Graph(src, dst, n, chunk=chunk).to(DEV)
        assert (g.csc.n_long > 0 and g.csr.n_long > 0) == (chunk == 8)
        _check_exact_forward(f"edges{chunk}", g, 17, 23)
        assert _C._lib.bot_last_kernel().decode() == "bot::spmm_softmax_kernel<q,1,32,1>"


def test_forward_exact_regimes_on_the_hub_graph():
    g, indptr, indices = _hub()
    x = _ints(g.number_of_nodes(), 40, 5)
    xd = torch.from_numpy(x).to(DEV)
    for relu in (False, True):
        o, l, q = _C.spmm_softmax(g.csc, xd, _beta(0.0), relu, 0.0, True)
        assert _same_bytes(o, torch.from_numpy(GC.mean32(indptr, indices, x, relu)).to(DEV))
        mx, _ = _C.spmm_max(g.csc, xd, relu)
        o, l, q = _C.spmm_softmax(g.csc, xd, _beta(128.0), relu, 0.0, True)
        assert _same_bytes(o, mx) and _same_bytes(q, mx * mx)
        o2, l2, q2 = _C.spmm_softmax(g.csc, xd, _beta(128.0), relu, 0.0, True)
        assert _same_bytes(o2, o) and _same_bytes(l2, l) and _same_bytes(q2, q)


# ------------------------------------------------------------------------------------------------ 2. backward, exact regime
def _perm_columns(n, F_, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(n) + 1 for _ in range(F_)], axis=1).astype(np.float32)


@pytest.mark.parametrize("F_", WIDTHS)
def test_backward_exact_regime(F_):
    """beta = 128, no parallel edges, every column of x a permutation of 1 .. n_src: the maximum is unique, lse = 128 max exactly and dx
    is the max backward of the restatement, bit for bit."""
    for name, g in _simple_graphs():
        indptr, indices = SG.csc_of(g)
        n_src, n_dst = g.number_of_src_nodes(), g.number_of_dst_nodes()
        x = _perm_columns(n_src, F_, F_ + len(name))
        dout = _ints(n_dst, F_, 5 * F_ + 1)
        for relu in (False, True):
            want = GC.max_backward64(indptr, indices, n_src, x, relu, dout)
            for pad in (0, 3, 4):
                xd, dd = _slab(x, pad), _slab(dout, pad)
                o, l, _ = _forward(g, xd, 128.0, relu, False, pad)
                mx, _ = _C.spmm_max(g.csc, xd, relu)
                assert _same_bytes(o, mx) and _same_bytes(l, mx * 128.0), (name, F_, relu, pad)
                buf = torch.full((n_src, F_ + pad), 9.0, device=DEV)[:, :F_] if pad else None
                dx = _C.spmm_softmax_bwd(g.csr, xd, _beta(128.0), relu, 0.0, dd, o, l, dx=buf)
                assert np.array_equal(dx.cpu().double().numpy(), want), (name, F_, relu, pad)
                if pad:
                    assert dx.data_ptr() == buf.data_ptr() and bool((dx._base[:, F_:] == 9.0).all())
                assert _same_bytes(_C.spmm_softmax_bwd(g.csr, xd, _beta(128.0), relu, 0.0, dd, o, l), dx)
    assert "spmm_softmax_bwd_kernel" in _C._lib.bot_last_kernel().decode()


# ------------------------------------------------------------------------------------------------ 3. normal inputs, toleranced
def _check_normal(name, g, F_, beta, relu, seed, rows=None, src_rows=None):
    """Forward (out, lse, q), the tensor form, and the backward sweep against float64 on standard-normal inputs; `rows` / `src_rows`:
    compare these destination / source rows only (the hub graph)."""
    indptr, indices = SG.csc_of(g)
    n_src, n_dst = g.number_of_src_nodes(), g.number_of_dst_nodes()
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n_src, F_)).astype(np.float32)
    dout = rng.standard_normal((n_dst, F_)).astype(np.float32)
    xd, dd = torch.from_numpy(x).to(DEV), torch.from_numpy(dout).to(DEV)
    res = GC.forward64(indptr, indices, x, beta, relu, EPS, rows)
    tol = GC.forward_bounds(res, beta, _exp_error())
    pick = (lambda t: t) if rows is None else (lambda t: t[rows])
    o, l, q = _C.spmm_softmax(g.csc, xd, _beta(beta), relu, EPS, True)
    for key, got in (("out", o), ("lse", l), ("q", q)):
        err = np.abs(pick(got.cpu().double().numpy()) - res[key])
        bad = _ratio(f"forward {key}", err, tol[key])
        assert bad.size == 0, (name, F_, beta, relu, key, bad[:5].tolist(), float(err.max()))
    t = ops.copy_u_softmax(g, xd, _beta(beta), relu=relu, eps=EPS, impl="tensor")
    for key, a, b in (("tensor form against float64", t.cpu().double().numpy(), None), ("kernel against tensor form", o.cpu().double().numpy(), t.cpu().double().numpy())):
        err = np.abs(pick(a) - (res["out"] if b is None else pick(b)))
        bad = _ratio(key, err, tol["out"])
        assert bad.size == 0, (name, F_, beta, relu, key, bad[:5].tolist(), float(err.max()))
    # the backward sweep on the float32 operands it gets: the forward's own out and lse
    dx = _C.spmm_softmax_bwd(g.csr, xd, _beta(beta), relu, EPS, dd, o, l)
    want, tol_dx = GC.backward64(g.csr.indptr.cpu().numpy(), g.csr.indices.cpu().numpy(), x, beta, relu, EPS, dout, o.cpu().numpy(),
                                 l.cpu().numpy(), _exp_error(), src_rows)
    got = dx.cpu().double().numpy()
    err = np.abs((got if src_rows is None else got[src_rows]) - want)
    bad = _ratio("backward dx", err, tol_dx)
    assert bad.size == 0, (name, F_, beta, relu, bad[:5].tolist(), float(err.max()))
    assert _same_bytes(_C.spmm_softmax_bwd(g.csr, xd, _beta(beta), relu, EPS, dd, o, l), dx)


@pytest.mark.parametrize("F_", WIDTHS + (17,))
def test_normal_inputs_against_fp64_restatement(F_):
    for i, (name, g) in enumerate(_graphs()):
        for j, beta in enumerate(BETAS):
            _check_normal(name, g, F_, beta, (i + j) % 2 == 0, 7 * F_ + i)
        _check_normal(name, g, F_, 1.0, i % 2 == 0, 11 * F_ + i)     # beta = 1 with the other relu setting


def test_normal_inputs_on_the_hub_graph():
    g, indptr, indices = _hub()
    deg = np.diff(indptr)
    rows = np.unique(np.concatenate([np.nonzero(deg > 2048)[0], np.arange(0, len(deg), 97)]))
    out_deg = np.diff(g.csr.indptr.cpu().numpy())
    src_rows = np.unique(np.concatenate([np.argsort(out_deg)[-3:], np.arange(0, len(out_deg), 997)]))
    assert int(deg[rows].max()) > 2048 and int(out_deg[src_rows].max()) > 2048
    _check_normal("hub", g, 40, 1.0, True, 3, rows, src_rows)


# ------------------------------------------------------------------------------------------------ 4. the op
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", [(5,), (41,), (64,), (3, 4)])
def test_copy_u_softmax_gradients_against_fp64(relu, shape):
    """x.grad under the suite's criterion; beta.grad - a one-element sum - under the bound derived from the forward's (GC.dbeta_bound)."""
    for name, g in (_graphs()[3], _graphs()[5], _graphs()[6]):
        indptr, indices = SG.csc_of(g)
        n_src, n_dst = g.number_of_src_nodes(), g.number_of_dst_nodes()
        gen = torch.Generator().manual_seed(1)
        x = torch.randn((n_src,) + shape, generator=gen).to(DEV).requires_grad_()
        beta = torch.tensor([0.8], device=DEV, requires_grad=True)
        out = ops.copy_u_softmax(g, x, beta, relu=relu, eps=EPS)
        assert out.shape == (n_dst,) + shape
        assert "spmm_softmax_kernel<q," in _C._lib.bot_last_kernel().decode()
        dout = torch.randn(out.shape, generator=gen)
        out.backward(dout.to(DEV))
        x2, d2 = x.detach().cpu().reshape(n_src, -1).numpy(), dout.reshape(n_dst, -1).numpy()
        b32 = float(np.float32(0.8))
        res = GC.forward64(indptr, indices, x2, b32, relu, EPS)
        tol = GC.forward_bounds(res, b32, _exp_error())
        assert _ratio("forward out", np.abs(out.detach().cpu().double().reshape(n_dst, -1).numpy() - res["out"]), tol["out"]).size == 0
        dx, _ = GC.backward64(g.csr.indptr.cpu().numpy(), g.csr.indices.cpu().numpy(), x2, b32, relu, EPS, d2, res["out"], res["lse"], 0.0)
        grad_close(x.grad.reshape(n_src, -1), dx)
        err, bound = abs(float(beta.grad) - GC.dbeta64(res, d2)), GC.dbeta_bound(res, tol, d2)
        RATIOS["dbeta"] = max(RATIOS.get("dbeta", 0.0), err / bound)
        assert err <= bound, (name, shape, relu, float(beta.grad), GC.dbeta64(res, d2), bound)
        # a float beta: no q, no beta gradient, the same out
        xf = x.detach().clone().requires_grad_()
        out_f = ops.copy_u_softmax(g, xf, b32, relu=relu, eps=EPS)
        assert "spmm_softmax_kernel<q," not in _C._lib.bot_last_kernel().decode() and _same_bytes(out_f.detach(), out.detach())
        out_f.backward(dout.to(DEV))
        assert _same_bytes(xf.grad, x.grad)


def test_the_csr_is_built_only_for_the_features_gradient():
    g = SG.small_graph(20, 30, 8).to(DEV)
    beta = torch.tensor([1.0], device=DEV, requires_grad=True)
    ops.copy_u_softmax(g, torch.randn(30, 4, device=DEV), beta).sum().backward()
    assert g._csr is None and beta.grad is not None
    x = torch.randn(30, 4, device=DEV, requires_grad=True)
    ops.copy_u_softmax(g, x).sum().backward()
    assert g._csr is not None and x.grad is not None
    with torch.no_grad():                                            # no gradient can be asked for: q is not produced
        ops.copy_u_softmax(g, x, beta)
    assert "spmm_softmax_kernel<4," in _C._lib.bot_last_kernel().decode()
    ops.copy_u_softmax(g, x, beta)
    assert "spmm_softmax_kernel<q,4," in _C._lib.bot_last_kernel().decode()


def test_isolated_destinations_and_sources():
    name, g = _graphs()[5]                                           # the block: isolated destinations, and sources without out-edges
    indptr, _ = SG.csc_of(g)
    x = torch.randn(g.number_of_src_nodes(), 12, device=DEV, requires_grad=True)
    beta = torch.tensor([1.0], device=DEV, requires_grad=True)
    out = ops.copy_u_softmax(g, x, beta, relu=True, eps=EPS)
    empty = torch.from_numpy(np.diff(indptr) == 0).to(DEV)
    assert int(empty.sum()) > 0 and bool((out[empty] == 0).all())
    o, l, q = _C.spmm_softmax(g.csc, x.detach(), beta.detach(), True, EPS, True)
    assert bool((l[empty] == 0).all()) and bool((q[empty] == 0).all())
    out.backward(torch.randn(out.shape, device=DEV))
    assert bool(torch.isfinite(x.grad).all()) and bool(torch.isfinite(beta.grad).all())
    unused = torch.from_numpy(np.diff(g.csr.indptr.cpu().numpy()) == 0).to(DEV)
    assert int(unused.sum()) > 0 and bool((x.grad[unused] == 0).all())


def test_nan_and_inf_stay_inside_the_rows_that_gather_them():
    name, g = _graphs()[4]                                           # long rows: the chunks and both combines
    indptr, indices = SG.csc_of(g)
    n = g.number_of_nodes()
    rng = np.random.default_rng(1)
    x = rng.standard_normal((n, 12)).astype(np.float32)
    dout = rng.standard_normal((n, 12)).astype(np.float32)
    bad = np.zeros_like(x, dtype=bool)
    bad[::17, ::2] = True
    bad[1::17, 1::2] = True
    poisoned = x.copy()
    poisoned[::17, ::2] = np.nan
    poisoned[1::17, 1::2] = np.inf
    clean = np.where(bad, np.float32(0), x)
    hit_dst = np.zeros((n, 12), dtype=bool)                            # (v, f) that gather a non-finite entry
    for v in range(n):
        hit_dst[v] = bad[indices[indptr[v]:indptr[v + 1]]].any(0)
    csr_p, csr_i = g.csr.indptr.cpu().numpy(), g.csr.indices.cpu().numpy()
    hit_src = bad.copy()                                               # (u, f): its own entry, or an out-edge into a poisoned (v, f)
    for u in range(n):
        hit_src[u] |= hit_dst[csr_i[csr_p[u]:csr_p[u + 1]]].any(0)
    assert 0 < hit_dst.mean() < 0.9 and 0 < hit_src.mean() < 0.95
    dd = torch.from_numpy(dout).to(DEV)
    for relu in (False, True):
        runs = []
        for vals in (poisoned, clean):
            xd = torch.from_numpy(vals).to(DEV)
            o, l, q = _C.spmm_softmax(g.csc, xd, _beta(1.0), relu, EPS, True)
            dx = _C.spmm_softmax_bwd(g.csr, xd, _beta(1.0), relu, EPS, dd, o, l)
            torch.cuda.synchronize()
            runs.append([t.cpu().numpy() for t in (o, l, q, dx)])
        for k in range(3):
            assert np.array_equal(runs[0][k][~hit_dst], runs[1][k][~hit_dst]) and np.isfinite(runs[0][k][~hit_dst]).all()
        assert np.array_equal(runs[0][3][~hit_src], runs[1][3][~hit_src]) and np.isfinite(runs[0][3][~hit_src]).all()


# ------------------------------------------------------------------------------------------------ 5. GENConv and DeeperGCN
@pytest.mark.parametrize("kw", [dict(), dict(msg_norm=True, learn_msg_scale=True), dict(mlp_layers=2), dict(learn_beta=True, beta=0.5),
                                dict(mlp_layers=2, msg_norm=True, learn_beta=True)])
@pytest.mark.parametrize("fin,fout", [(3, 16), (41, 16)])
def test_genconv_against_fp64_restatement(kw, fin, fout):
    GC.check_conv(_parent(), DEV, fin, fout, **kw)
    GC.check_conv(_block(), DEV, fin, fout, seed=1, **kw)
    g = _parent()
    sub = g.subgraph(torch.randperm(g.number_of_nodes(), generator=torch.Generator().manual_seed(4))[:1500])
    GC.check_conv(sub, DEV, fin, fout, seed=2, **kw)


def test_genconv_on_isolated_destinations_and_with_edge_features():
    GC.check_conv(_graphs()[3][1], DEV, 6, 4, learn_beta=True)
    GC.check_conv(_graphs()[3][1], DEV, 6, 4, edge_feats=True, learn_beta=True)
    GC.check_conv(_block(), DEV, 5, 5, edge_feats=True, seed=1)


def test_genconv_runs_the_kernel_form():
    g = _parent()
    calls = []
    real = _C.spmm_softmax
    _C.spmm_softmax = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        bnn.GENConv(8, 8).to(DEV)(g, g.ndata["feat"])
    finally:
        _C.spmm_softmax = real
    assert calls == [1]


@pytest.mark.parametrize("kw", [dict(), dict(learn_beta=True, msg_norm=True, mlp_layers=2, beta=0.5)])
def test_deepergcn_against_fp64_restatement(kw):
    from tests import block_cases as BC
    g = BC.parent_graph(DEV, n=3000, e_raw=22000)
    torch.manual_seed(3)
    GC.check_stack(bnn.DeeperGCN(8, 5, 12, 3, dropout=0.5, **kw), g, g.ndata["feat"].cpu(), DEV)
    sub = g.subgraph(torch.randperm(3000, generator=torch.Generator().manual_seed(5))[:1200])
    GC.check_stack(bnn.DeeperGCN(8, 5, 12, 3, **kw), sub, sub.ndata["feat"].cpu(), DEV)
    nids = torch.randperm(3000, generator=torch.Generator().manual_seed(3))[:600]
    _, _, blocks = next(iter(NodeDataLoader(g, nids, MultiLayerNeighborSampler([5, 7, 9]), batch_size=600, seed=4)))
    GC.check_stack(bnn.DeeperGCN(8, 5, 12, 3, **kw), blocks, blocks[0].srcdata["feat"].cpu(), DEV)


def test_build_gen_full_batch_step():
    wl = workloads.build_gen("arxiv", DEV, scale=0.05)
    res = wl.step()
    assert all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in res[3:6])
    params = dict(wl.model.named_parameters())
    assert "convs.1.beta" in params
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params.values())


def test_build_gen_sampled_epoch():
    wl = workloads.build_gen("arxiv", DEV, sampled=True, scale=0.05)
    assert len(wl.loader) == workloads.SAMPLED["arxiv"][1]
    loss = wl.epoch()
    assert np.isfinite(float(loss))
    params = dict(wl.model.named_parameters())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params.values()) and params["convs.0.beta"].grad is not None


def test_report_measured_figures():
    """Prints what the README section quotes (run after the tests above in file order; it asserts what they asserted: no ratio above 1)."""
    print(f"exponential: {_exp_error():.3e} relative ({_exp_error() / GC.U:.2f} U)")
    for k, v in sorted(RATIOS.items()):
        print(f"largest error / bound, {k}: {v:.4f}")
    assert all(v <= 1.0 for v in RATIOS.values())
