"""Edge weights on the MI355X: one `bot_propagate_step_w_f32` sweep (csrc/propagate.hip) against the float64 restatement of one weighted
step, full weighted `LabelPropagation` / `CorrectAndSmooth` runs, `bot_subgraph_tally_i32` and `sampling.saint_norms` against their numpy
restatements integer for integer / bit for bit, and `nn.GraphConv` / `nn.GCN` with weights on the real kernels
(tests/edge_weight_cases.py holds the restatements)."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bot_amd
from bot_amd import _C, minibatch, sampling, smoothing, synth, workloads
from bot_amd import nn as bnn
from tests import edge_weight_cases as EW
from tests import sage_cases as SG
from tests import smooth_cases as SC
from tests import subgraph_cases as SGC
from tests.parity_cases import fwd_close, grad_close
from tests.test_smooth_gpu import _COMBOS, _GRAPHS, _gpu_graph, _view

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = 1.0e-5             # full runs: absolute, against the float64 restatement (tests/test_smooth_gpu.py's criterion)
U = 2.0 ** -24           # unit roundoff of float32


def _hub():
    if "hub" not in _GRAPHS:
        from tests.test_subgraph_gpu import _hub_graph
        _GRAPHS["hub"] = _hub_graph()
    return _GRAPHS["hub"]


# ------------------------------------------------------------------------------------------------ 1. one weighted step
def _raw_step_w(d, y, y0, out, alpha, beta, ss, ds, lo, hi, fixed, row_abs, out_scale, ew):
    """bot_propagate_step_w_f32 itself (the wrapper calls it only with a weight): `ew` may be None = NULL."""
    n, C = y.shape
    partial = torch.empty(d.n_slots * C, dtype=torch.float32, device=y.device) if d.n_long else None
    p = _C._ptr
    rc = _C._lib.bot_propagate_step_w_f32(
        d.indptr.data_ptr(), d.indices.data_ptr(), n, d.nnz, d.items.data_ptr(), d.n_items, p(d.long_rows), p(d.long_ptr), d.n_long,
        y.data_ptr(), _C._ld(y), y0.data_ptr(), _C._ld(y0), out.data_ptr(), _C._ld(out), C, float(alpha), float(beta), p(ss), p(ds),
        float(lo), float(hi), p(fixed), p(row_abs), p(out_scale), p(partial), p(ew), _C._stream())
    assert rc == 0, _C._lib.bot_last_error()
    return out


def _check_step_w(g, src, dst, C, *, strided, fixed, row_abs, clamp, adj, seed, out_scale=False):
    """One weighted launch against EW.step in float64.  Bound per entry: tests/test_smooth_gpu.py::_check_step's chain - deg fused
    multiply-adds, one product for alpha * dst_scale, one for beta * y0, one more fma - plus ONE more rounding per term, the product
    fl(ew * src_scale) the lane forms before the broadcast: |error| <= (deg + 9) 2^-24 (alpha dst_scale sum |ew src_scale y| + |beta y0|).
    The out_scale and row_abs terms are as there.  Weights: uniform in [0, 2), about a tenth exactly 0."""
    n = g.number_of_nodes()
    d = g.csc
    gen = torch.Generator().manual_seed(seed)
    y, _, _ = _view(n, C, strided, True, gen)
    y0, _, _ = _view(n, C, (strided + 1) % 3 if strided else 0, True, gen)
    out, out_base, off = _view(n, C, strided, False, gen)
    E = src.numel()
    w = 2.0 * torch.rand(E, generator=gen)
    w[torch.rand(E, generator=gen) < 0.1] = 0.0
    assert E == 0 or n < 8 or int((w == 0).sum()) > 0
    deg = torch.bincount(dst, minlength=n)
    degf = deg.float().clamp(min=1)
    ss, ds = {"DAD": (degf ** -0.5, degf ** -0.5), "DA": (None, 1.0 / degf), "AD": (1.0 / degf, None), None: (None, None)}[adj]
    fx = (torch.rand(n, generator=gen) < 0.3) if fixed else None
    lo, hi = (-0.25, 0.5) if clamp else (-math.inf, math.inf)
    alpha, beta = 0.8, 0.2
    ref, ref_abs, mag = EW.step(src, dst, w, y.cpu(), y0.cpu(), alpha, beta, ss, ds, lo, hi, fx)
    dv = lambda t: None if t is None else t.to(DEV).contiguous()
    ew = w.to(DEV)[d.eid.long()].contiguous()                      # CSC position order
    ra = torch.full((n,), -1.0, device=DEV) if row_abs else None
    osc = (0.5 + torch.rand(n, generator=gen)) if out_scale else None
    kw = dict(fixed=None if fx is None else dv(fx.to(torch.uint8)), out_scale=dv(osc))
    got = _C.propagate_step(d, y, y0, out, alpha, beta, dv(ss), dv(ds), lo, hi, row_abs=ra, ew=ew, **kw)
    assert got is out
    kernel = _C._lib.bot_last_kernel().decode()
    o = out.cpu().double()
    tol = (deg.double()[:, None] + 9) * U * mag
    want = ref if osc is None else ref * osc.double()[:, None]
    tol_o = tol if osc is None else tol * osc.double()[:, None] + U * want.abs()
    err = (o - want).abs()
    bad = err > tol_o
    print(f"weighted step n={n} C={C} {adj} strided={strided}: max |diff| = {err.max().item() if err.numel() else 0.0:.3e}, "
          f"largest |diff| / bound = {(err / tol_o.clamp(min=1e-300)).max().item() if err.numel() else 0.0:.3f}")
    assert not bool(bad.any()), (C, adj, torch.nonzero(bad)[:5].tolist(), err.max().item())
    if fx is not None:
        assert torch.equal(out.cpu()[fx], y0.cpu()[fx] if osc is None else y0.cpu()[fx] * osc[fx][:, None])
    if clamp and fx is None and osc is None:
        assert o.min() >= lo and o.max() <= hi
    back = out_base.cpu()                                           # nothing outside the [n, C] view was written
    back[:, off:off + C] = 777.0
    assert bool((back == 777.0).all())
    if row_abs:
        tol_abs = tol.sum(1) + (C + 8) * U * ref_abs
        assert bool(((ra.cpu().double() - ref_abs).abs() <= tol_abs).all()), (C, adj, (ra.cpu().double() - ref_abs).abs().max().item())
    # two calls give identical bytes
    out2 = torch.empty_like(out_base)[:, off:off + C]
    ra2 = torch.empty(n, device=DEV) if row_abs else None
    _C.propagate_step(d, y, y0, out2, alpha, beta, dv(ss), dv(ds), lo, hi, row_abs=ra2, ew=ew, **kw)
    assert torch.equal(out2.view(torch.int32), out.view(torch.int32))
    if row_abs:
        assert torch.equal(ra2.view(torch.int32), ra.view(torch.int32))
    # ew = ones, and ew = NULL through the weighted entry: the bytes of the unweighted entry point
    plain = torch.empty_like(out_base)[:, off:off + C]
    ra_p = torch.empty(n, device=DEV) if row_abs else None
    _C.propagate_step(d, y, y0, plain, alpha, beta, dv(ss), dv(ds), lo, hi, row_abs=ra_p, **kw)
    assert "ew" not in _C._lib.bot_last_kernel().decode()
    for unit in (torch.ones(E, device=DEV), None):
        o1 = torch.empty_like(out_base)[:, off:off + C]
        ra1 = torch.empty(n, device=DEV) if row_abs else None
        if unit is None:
            _raw_step_w(d, y, y0, o1, alpha, beta, dv(ss), dv(ds), lo, hi, kw["fixed"], ra1, kw["out_scale"], None)
            assert "ew" not in _C._lib.bot_last_kernel().decode()
        else:
            _C.propagate_step(d, y, y0, o1, alpha, beta, dv(ss), dv(ds), lo, hi, row_abs=ra1, ew=unit, **kw)
        assert torch.equal(o1.view(torch.int32), plain.view(torch.int32))
        if row_abs:
            assert torch.equal(ra1.view(torch.int32), ra_p.view(torch.int32))
    return kernel


@pytest.mark.parametrize("C", [1, 3, 4, 40, 47, 260, 1024])
def test_weighted_step_kernel_against_fp64_restatement_of_one_step(C):
    """The 300-row fixture at every lane width (4- / 8- / 16-byte lanes, groups of 8 .. 64 lanes) and chunk count (1 .. 16)."""
    src, dst, n = SC.graph("tiny")
    g = _gpu_graph("tiny")
    kernels = {_check_step_w(g, src, dst, C, seed=100 + C + i, **kw) for i, kw in enumerate(_COMBOS)}
    assert all(k.startswith("bot::prop_step_kernel<") and k.endswith(",ew>") for k in kernels), kernels
    if C % 4 == 0:
        assert len(kernels) == 2, kernels               # the odd-pitch slice takes 4-byte lanes, the others 16-byte lanes


def test_weighted_step_kernel_on_the_edge_case_graph_at_32_lanes():
    """The one group width the widths above leave out for the weighted instances (17 columns of 4-byte lanes: groups of 32), on
    SG.sweep_edges: with chunk = 8 its rows above 8 in-edges run as chunks of a long row, each chunk with its own weights; with
    chunk = 128 the rows of 63 / 64 / 65 in-edges are walked whole, 32 ids at a time."""
    src, dst, n = SG.sweep_edges()
    for chunk in (8, 128):
        g = bot_amd.Graph(src, dst, n, chunk=chunk).to(DEV)
        assert (g.csc.n_long > 0) == (chunk == 8)
        kernels = {_check_step_w(g, src, dst, 17, seed=300 + i, **kw) for i, kw in enumerate(_COMBOS)}
        assert kernels == {"bot::prop_step_kernel<1,32,1,ew>"}, kernels


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_weighted_step_kernel_against_fp64_restatement_row_counts(n):
    src, dst = SC.powerlaw_graph(n, 4 * n, 40 + n, n_isolated=1)
    g = bot_amd.Graph(src, dst, n).to(DEV)
    for C in (3, 40):
        for i, kw in enumerate(_COMBOS):
            _check_step_w(g, src, dst, C, seed=200 + n + C + i, **kw)


@pytest.mark.parametrize("combo", [0, 2])
def test_weighted_step_kernel_against_fp64_restatement_on_the_hub_graph(combo):
    """Largest in-degree above 2048: the hub rows run as chunks of the row plan, each chunk with its own weights, combined in slot order."""
    g = _hub()
    src, dst = (t.cpu() for t in g.edges())
    assert int(torch.bincount(dst).max()) > 2048 and g.csc.n_long > 0
    _check_step_w(g, src, dst, 8, seed=8 + combo, **_COMBOS[combo])


# ------------------------------------------------------------------------------------------------ 2. full weighted runs
@pytest.mark.parametrize("adj", ["DAD", "DA"])
@pytest.mark.parametrize("C", [7, 40])
def test_weighted_correct_and_smooth_and_label_propagation_against_fp64_restatement(C, adj):
    """50 + 50 iterations at alpha 0.8 on the 3 000-node fixture with weights uniform in [0.5, 1.5): the kernel form within 1.0e-5
    absolute of the float64 restatement, and of the tensor form on the GPU; the weight as a tensor and as an edata key."""
    g = _gpu_graph("small")
    w = EW.weights("small").to(DEV)
    y_soft, y_true, mask = (t.to(DEV) for t in SC.cs_inputs("small", C))
    for autoscale in (True, False):
        ref, raw = EW.cs_reference("small", C, adj, autoscale)
        assert SC.scale_margin(raw) > 0.01, "a raw autoscale factor lies within 1 % of the threshold: choose another seed"
        kw = dict(correction_adj=adj, smoothing_adj=adj, autoscale=autoscale)
        got = smoothing.CorrectAndSmooth(impl="kernel", **kw)(g, y_soft, y_true, mask, edge_weight=w)
        ten = smoothing.CorrectAndSmooth(impl="tensor", **kw)(g, y_soft, y_true, mask, edge_weight=w)
        err, err_t = (got.cpu().double() - ref).abs().max().item(), (got - ten).abs().max().item()
        print(f"weighted C&S small C={C} {adj} autoscale={autoscale}: kernel max |diff| = {err:.3e}, kernel vs tensor form {err_t:.3e}")
        assert got.is_cuda and got.dtype == torch.float32 and got.shape == y_soft.shape and err <= TOL and err_t <= TOL
        assert torch.equal(smoothing.CorrectAndSmooth(impl="kernel", **kw)(g, y_soft, y_true, mask, edge_weight=w), got)
    labels, ref = EW.lp_reference("small", C, adj)
    g.edata["w_test"] = w.view(-1, 1)
    try:
        got = smoothing.LabelPropagation(50, 0.8, adj, impl="kernel")(g, labels.to(DEV), mask=mask, edge_weight="w_test")
    finally:
        del g.edata["w_test"]
    ten = smoothing.LabelPropagation(50, 0.8, adj, impl="tensor")(g, labels.to(DEV), mask=mask, edge_weight=w)
    err, err_t = (got.cpu().double() - ref).abs().max().item(), (got - ten).abs().max().item()
    print(f"weighted LP small C={C} {adj}: kernel max |diff| = {err:.3e}, kernel vs tensor form {err_t:.3e}")
    assert err <= TOL and err_t <= TOL
    assert smoothing.default_impl(y_soft, weighted=True) in ("kernel", "tensor")


def test_weighted_runs_follow_an_in_place_change_and_make_no_host_read():
    src, dst, n = SC.graph("small")
    g = _gpu_graph("small")
    w = EW.weights("small").to(DEV).clone()
    y_soft, y_true, mask = (t.to(DEV) for t in SC.cs_inputs("small", 7))
    for impl in ("kernel", "tensor"):
        cs = smoothing.CorrectAndSmooth(5, 0.8, "DAD", 5, 0.8, "DA", autoscale=False, impl=impl)
        a = cs(g, y_soft, y_true, mask, edge_weight=w)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            again = cs.smooth(g, cs.correct(g, y_soft, y_true, mask, w), y_true, mask, w)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        assert torch.equal(again, a)
        w[::2] *= 3.0                                               # in place: the cached copies are prepared again
        b = cs(g, y_soft, y_true, mask, edge_weight=w)
        c = EW.propagate                                            # (two adjacencies: the two stages restated one by one)
        idx = mask.cpu()
        E0 = torch.zeros(n, 7, dtype=torch.float64)
        E0[idx] = SC.onehot(y_true.cpu(), 7) - y_soft.cpu().double()[idx]
        cor = y_soft.cpu().double() + c(src, dst, n, w.cpu(), E0, 5, 0.8, "DAD", (idx, "fix"))
        cor[idx] = SC.onehot(y_true.cpu(), 7)
        want = c(src, dst, n, w.cpu(), cor, 5, 0.8, "DA", "clamp01")
        assert not torch.equal(a, b) and (b.cpu().double() - want).abs().max().item() <= TOL
        w[::2] /= 3.0


# ------------------------------------------------------------------------------------------------ 3. the tally
def _tally_graphs():
    one = bot_amd.Graph(torch.tensor([0]), torch.tensor([0]), 1).to(DEV)
    rs, rd = synth.powerlaw_edges(65, 400, 3)
    g65 = bot_amd.preprocess(bot_amd.Graph(rs, rd, 65)).to(DEV)
    rs, rd = synth.powerlaw_edges(300, 2500, 1)
    g300 = bot_amd.preprocess(bot_amd.Graph(rs, rd, 300)).to(DEV)
    return {"1": one, "65": g65, "300": g300}


@pytest.mark.parametrize("name", ["1", "65", "300", "hub"])
def test_subgraph_tally_bit_exact_against_the_numpy_restatement(name):
    """Integer for integer: empty set, one node, all nodes, a random third, and (the hub graph: a row above 2 048 positions, the
    workgroup kernel) the hub with its neighbourhood; three sets tallied in a row accumulate; the node map is all -1 afterwards."""
    g = _hub() if name == "hub" else _tally_graphs()[name]
    n = g.number_of_nodes()
    indptr, indices, _ = SGC.csc_arrays(g)
    rng = np.random.default_rng(n)
    third = np.union1d(rng.permutation(n)[: n // 3], [n // 2])       # (with the single node: its self-loop is tallied by three sets)
    sets = [np.zeros(0, dtype=np.int64), np.array([n // 2]), np.arange(n), third]
    deg = np.diff(indptr)
    hub = int(np.argmax(deg))
    if name == "hub":
        assert deg[hub] > SGC.LONG_TILE
        sets.append(np.unique(np.concatenate([[hub], indices[indptr[hub]:indptr[hub + 1]]])))
        sets.append(np.unique(np.concatenate([[hub], rng.permutation(n)[:50]])))          # the long row with few sources kept
    node_map = sampling._node_map(g)
    acc = torch.zeros(g.csc.nnz, dtype=torch.int32, device=DEV)
    acc_ref = np.zeros(g.csc.nnz, dtype=np.int32)
    for s in sets:
        nodes = torch.from_numpy(s).to(DEV, torch.int32).contiguous()
        t = torch.zeros(g.csc.nnz, dtype=torch.int32, device=DEV)
        assert _C.subgraph_tally(g.csc, nodes, node_map, t) is t
        want = EW.tally_reference(indptr, indices, [s])
        assert np.array_equal(t.cpu().numpy(), want), (name, len(s))
        assert bool((node_map == -1).all())
        _C.subgraph_tally(g.csc, nodes, node_map, acc)
        acc_ref += want
        assert np.array_equal(acc.cpu().numpy(), acc_ref)                                 # the sets accumulate
    assert int(acc_ref.max()) >= 3 or n == 1
    if n > 1:
        assert _C._lib.bot_last_kernel().decode() == "subgraph_unmark_kernel"


def test_saint_norms_bit_exact_against_the_numpy_restatement():
    rs, rd = synth.powerlaw_edges(300, 2500, 1)
    g = bot_amd.preprocess(bot_amd.Graph(rs, rd, 300)).to(DEV)
    for sampler in (sampling.SAINTSampler("walk", (10, 2)), sampling.SAINTSampler("node", 40)):
        lw, en = sampling.saint_norms(g, sampler, 40, seed=5)
        want_lw, want_en, _, count, T = EW.saint_norms_reference(g, sampler, 40, seed=5)
        assert torch.equal(lw, sampling.saint_loss_weights(g, sampler, 40, seed=5))
        assert np.array_equal(lw.cpu().numpy(), want_lw)
        assert en.is_cuda and en.dtype == torch.float32 and np.array_equal(en.cpu().numpy(), want_en)
        assert float(en.min()) >= 1.0 and float(en.max()) <= 40.0 and int((T > 0).sum()) > 0
        assert bool((sampling._node_map(g) == -1).all())


# ------------------------------------------------------------------------------------------------ 4. GraphConv / GCN on the real kernels
@pytest.mark.parametrize("fin,fout", [(3, 16), (16, 3), (41, 16), (16, 41)])
@pytest.mark.parametrize("norm", ["both", "right", "none"])
def test_graphconv_edge_weight_against_fp64_restatement(norm, fin, fout):
    rs, rd = synth.powerlaw_edges(300, 2500, 1)
    g = bot_amd.preprocess(bot_amd.Graph(rs, rd, 300))
    src, dst = g.edges()
    n, E = g.number_of_nodes(), g.number_of_edges()
    gd = g.to(DEV)
    gen = torch.Generator().manual_seed(fin * 100 + fout)
    torch.manual_seed(1)
    conv = bnn.GraphConv(fin, fout, norm=norm).to(DEV)
    feat = torch.randn(n, fin, generator=gen)
    ew = 0.25 + 1.5 * torch.rand(E, generator=gen)
    dout = torch.randn(n, fout, generator=gen)
    fd, ed = feat.to(DEV).requires_grad_(), ew.to(DEV).requires_grad_()
    seen = []
    real = _C.spmm

    def spy(d, x, w=None, *a, **k):
        out = real(d, x, w, *a, **k)
        seen.append((w is not None, _C._lib.bot_last_kernel().decode()))
        return out
    _C.spmm = spy
    try:
        out = conv(gd, fd, edge_weight=ed)
    finally:
        _C.spmm = real
    assert len(seen) == 1 and seen[0][0] and seen[0][1].startswith("bot::spmm"), seen         # a weighted SpMM ran
    assert not seen[0][1].startswith("bot::spmm_kernel<") or seen[0][1].endswith(",true>"), seen
    out.backward(dout.to(DEV))
    f64, e64 = feat.double().requires_grad_(), ew.double().requires_grad_()
    W64, b64 = conv.weight.detach().cpu().double().requires_grad_(), conv.bias.detach().cpu().double().requires_grad_()
    ref = EW.graphconv(src, dst, n, n, f64, W64, b64, e64, norm)
    ref.backward(dout.double())
    fwd_close(out, ref.detach().numpy())
    grad_close(fd.grad, f64.grad.numpy())
    grad_close(ed.grad, e64.grad.numpy())
    grad_close(conv.weight.grad, W64.grad.numpy())
    grad_close(conv.bias.grad, b64.grad.numpy())
    with torch.no_grad():
        fwd_close(conv(gd, fd, edge_weight=torch.ones(E, device=DEV)), conv(gd, fd).cpu().double().numpy())


def test_gcn_edge_weight_against_fp64_restatement_and_one_saint_step():
    from tests.test_edge_weight_host import _gcn, _gcn_reference
    rs, rd = synth.powerlaw_edges(300, 2500, 1)
    g = bot_amd.preprocess(bot_amd.Graph(rs, rd, 300))
    n, E = g.number_of_nodes(), g.number_of_edges()
    gen = torch.Generator().manual_seed(2)
    feat = torch.randn(n, 6, generator=gen)
    w = 0.25 + 1.5 * torch.rand(E, generator=gen)
    model = _gcn(6, 4).eval()
    ref = _gcn_reference(model, [g, g], feat, [w, w])
    with torch.no_grad():
        got = model.to(DEV)(g.to(DEV), feat.to(DEV), edge_weight=w.to(DEV))
    fwd_close(got, ref.numpy())
    # one GraphSAINT step with the aggregator normalisation
    wl = workloads.build_saint("cora", DEV, scale=0.25, aggregator_norm=True)
    assert wl.edge_weight == "saint_norm" and wl.graph.edata["saint_norm"].is_cuda
    seen = []
    real = _C.spmm

    def spy(d, x, w=None, *a, **k):
        seen.append(w is not None)
        return real(d, x, w, *a, **k)
    _C.spmm = spy
    try:
        out = None
        for sub in wl.loader:
            out = minibatch.subgraph_step(wl.model, sub, wl.optimizer, wl.labels, wl.roles, step_kw=wl.step_kw, loss_weight=wl.loss_weight,
                                          edge_weight=wl.edge_weight)
            if out is not None:
                break
    finally:
        _C.spmm = real
    assert out is not None and math.isfinite(float(out[0].detach())) and seen and all(seen)
