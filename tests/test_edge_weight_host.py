"""Edge weights without a GPU: `nn.GraphConv(edge_weight=)`, `nn.GCN(edge_weight=)` and `nn.EdgeWeightNorm` on the emulated backend
against their float64 restatements (tests/edge_weight_cases.py), weighted label propagation / Correct and Smooth on CPU tensors,
`sampling.saint_norms` over stand-ins for the kernels, `build_saint(aggregator_norm=True)`, and the new symbols' argument checks.
tests/test_edge_weight_gpu.py holds the kernels to the same restatements."""
import ctypes
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bot_amd
from bot_amd import nn as bnn
from bot_amd import sampling, smoothing, synth
from bot_amd.errors import DGLError
from bot_amd.graph import reorder_graph
from tests import edge_weight_cases as EW
from tests import saint_cases as SN
from tests import smooth_cases as SC
from tests import subgraph_cases as SGC
from tests.parity_cases import fwd_close, grad_close

F64 = torch.float64
TOL = 1.0e-5            # the full propagation runs: absolute, against the float64 restatement (tests/test_smooth_host.py's criterion)


def _graph(n=300, e_raw=2500, seed=1):
    rs, rd = synth.powerlaw_edges(n, e_raw, seed)
    return bot_amd.to_bidirected(bot_amd.Graph(rs, rd, n)).remove_self_loop().add_self_loop()


@pytest.fixture
def backend(monkeypatch):
    from bot_amd import _C
    from tests import _oracle_backend
    _oracle_backend.install(monkeypatch)
    monkeypatch.setattr(_C, "node_subgraph", SGC.node_subgraph_standin)
    monkeypatch.setattr(_C, "saint_walk", SN.saint_walk_standin)
    monkeypatch.setattr(_C, "saint_nodes", SN.saint_nodes_standin)
    monkeypatch.setattr(_C, "subgraph_tally", EW.subgraph_tally_standin)


# ------------------------------------------------------------------------------------------------ 1. GraphConv
def _conv_case(g, fin, fout, norm, ew, seed):
    """(layer, feat leaf, ew leaf or None, out) of the layer under test and (out, grads) of the float64 restatement."""
    src, dst = g.edges()
    n = g.number_of_nodes()
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    conv = bnn.GraphConv(fin, fout, norm=norm)
    with torch.no_grad():
        conv.bias.copy_(torch.randn(fout, generator=gen))
    feat = torch.randn(n, fin, generator=gen).requires_grad_()
    dout = torch.randn(n, fout, generator=gen)
    ewl = None if ew is None else ew.clone().requires_grad_()
    out = conv(g, feat) if ew is None else conv(g, feat, edge_weight=ewl)
    out.backward(dout)
    f64 = feat.detach().double().requires_grad_()
    W64, b64 = conv.weight.detach().double().requires_grad_(), conv.bias.detach().double().requires_grad_()
    e64 = None if ew is None else ew.double().reshape(-1).requires_grad_()
    ref = EW.graphconv(src, dst, n, n, f64, W64, b64, e64, norm)
    ref.backward(dout.double())
    return conv, feat, ewl, out, ref, (f64.grad, W64.grad, b64.grad, None if e64 is None else e64.grad)


@pytest.mark.parametrize("fin,fout", [(16, 5), (5, 16)])            # the GEMM before the aggregation, and after it
@pytest.mark.parametrize("norm", ["both", "right", "none"])
def test_graphconv_edge_weight_against_fp64_restatement(backend, norm, fin, fout):
    g = _graph()
    E = g.number_of_edges()
    gen = torch.Generator().manual_seed(5)
    for shape in ((E,), (E, 1)):
        ew = (0.25 + 1.5 * torch.rand(E, generator=gen)).reshape(shape)
        conv, feat, ewl, out, ref, (gf, gW, gb, ge) = _conv_case(g, fin, fout, norm, ew, seed=3)
        fwd_close(out, ref.detach().numpy())
        grad_close(feat.grad, gf.numpy())
        grad_close(conv.weight.grad, gW.numpy())
        grad_close(conv.bias.grad, gb.numpy())
        assert ewl.grad.shape == ew.shape
        grad_close(ewl.grad.reshape(-1), ge.numpy())
    # a constant weight: no gradient is asked of it, the others are the same
    conv2 = bnn.GraphConv(fin, fout, norm=norm)
    conv2.load_state_dict(conv.state_dict())
    f2 = feat.detach().clone().requires_grad_()
    conv2(g, f2, edge_weight=ew).sum().backward()
    assert ew.grad is None and f2.grad is not None
    # unit weights: the unweighted layer
    _, feat_u, _, out_u, ref_u, grads_u = _conv_case(g, fin, fout, norm, None, seed=3)
    _, feat_1, _, out_1, _, _ = _conv_case(g, fin, fout, norm, torch.ones(E), seed=3)
    fwd_close(out_1, ref_u.detach().numpy())
    fwd_close(out_1, out_u.detach().double().numpy())
    grad_close(feat_1.grad, grads_u[0].numpy())


def test_graphconv_edge_weight_errors(backend):
    g = _graph()
    E, n = g.number_of_edges(), g.number_of_nodes()
    conv = bnn.GraphConv(4, 4)
    feat = torch.randn(n, 4)
    with pytest.raises(DGLError):
        conv(g, feat, edge_weight=torch.ones(E - 1))
    with pytest.raises(DGLError):
        conv(g, feat, edge_weight=torch.ones(E, 2))
    with pytest.raises(DGLError):
        conv(g, feat, edge_weight=torch.ones(E, dtype=torch.float64))
    part = _graph(n=200, e_raw=1500, seed=7)
    part.halo = object()                                             # a partition's block carries a halo plan
    with pytest.raises(ValueError, match="partition"):
        conv(part, torch.randn(200, 4), edge_weight=torch.ones(part.number_of_edges()))
    with pytest.raises(ValueError, match="partition"):
        bnn.EdgeWeightNorm()(part, torch.ones(part.number_of_edges()))


# ------------------------------------------------------------------------------------------------ 2. the GCN stack
def _gcn(fin, C, n_layers=2):
    torch.manual_seed(11)
    return bnn.GCN(in_feats=fin, n_classes=C, n_hidden=8, n_layers=n_layers, activation=F.relu, norm="none", norm_adj="symm", use_linear=True)


def _gcn_reference(model, graphs, feat, weights):
    """The stack in float64 from the model's own parameters: layer i = graphconv(graphs[i]) + linear_i(destination prefix), ReLU between."""
    h = feat.double()
    for i, (g, w) in enumerate(zip(graphs, weights)):
        src, dst = g.edges()
        conv = model.convs[i]
        c = EW.graphconv(src, dst, g.number_of_src_nodes(), g.number_of_dst_nodes(), h, conv.weight.detach().double(), conv.bias.detach().double(),
                         None if w is None else w.double().reshape(-1), "both")
        h = c + h[:c.shape[0]] @ model.linear[i].weight.detach().double().t()
        if i < len(graphs) - 1:
            h = torch.relu(h)
    return h


def test_gcn_edge_weight_on_graph_subgraph_and_blocks_against_fp64_restatement(backend):
    g = _graph()
    n, E = g.number_of_nodes(), g.number_of_edges()
    gen = torch.Generator().manual_seed(2)
    feat = torch.randn(n, 6, generator=gen)
    model = _gcn(6, 4).eval()
    w = 0.25 + 1.5 * torch.rand(E, generator=gen)
    with torch.no_grad():
        out = model(g, feat, edge_weight=w)
        plain = model(g, feat)
        fwd_close(out, _gcn_reference(model, [g, g], feat, [w, w]).numpy())
        fwd_close(plain, _gcn_reference(model, [g, g], feat, [None, None]).numpy())
        fwd_close(model(g, feat, edge_weight=torch.ones(E)), plain.double().numpy())
        assert float((out - plain).abs().max()) > 1e-3                 # the weights reach the layers
        # a Subgraph: its own edge ids (CSC positions); the parent's rows arrive through edata
        g.edata["w"] = w
        nodes = torch.randperm(n, generator=gen)[:120]
        sub = sampling.node_subgraph(g, nodes)
        ws = sub.edata["w"]
        assert ws.shape == (sub.number_of_edges(),) and torch.equal(ws, w[sub.parent_eid.long()])
        fwd_close(model(sub, feat[nodes], edge_weight=ws), _gcn_reference(model, [sub, sub], feat[nodes], [ws, ws]).numpy())
        # a block list: one tensor per block
        s, d = g.edges()
        k0, k1 = d < 150, (s < 150) & (d < 60)
        b0 = bot_amd.Graph(s[k0], d[k0], n, num_dst_nodes=150)
        b1 = bot_amd.Graph(s[k1], d[k1], 150, num_dst_nodes=60)
        assert b0.is_block and b1.is_block
        w0, w1 = w[k0].contiguous(), w[k1].contiguous()
        for conv in model.convs:
            conv.set_allow_zero_in_degree(True)
        got = model([b0, b1], feat, edge_weight=[w0, w1])
        assert got.shape == (60, 4)
        fwd_close(got, _gcn_reference(model, [b0, b1], feat, [w0, w1]).numpy())
        with pytest.raises(ValueError, match="list of 2"):
            model([b0, b1], feat, edge_weight=[w0])
        with pytest.raises(ValueError, match="list of 2"):
            model([b0, b1], feat, edge_weight=w0)
        with pytest.raises(ValueError, match="one edge_weight tensor"):
            model(g, feat, edge_weight=[w, w])
        with pytest.raises(DGLError):
            model(g, feat, edge_weight=w[:-1])


# ------------------------------------------------------------------------------------------------ 3. EdgeWeightNorm
@pytest.mark.parametrize("norm", ["both", "right", "none"])
def test_edge_weight_norm_against_fp64_restatement(backend, norm):
    g = _graph()
    src, dst = g.edges()
    n, E = g.number_of_nodes(), g.number_of_edges()
    w = 0.1 + 2.0 * torch.rand(E, generator=torch.Generator().manual_seed(4))
    for eps in (0.0, 0.5):
        got = bnn.EdgeWeightNorm(norm, eps=eps)(g, w)
        assert got.dtype == torch.float32 and got.shape == (E,)
        want = EW.edge_weight_norm(src, dst, n, w, norm, eps)
        np.testing.assert_allclose(got.double().numpy(), want.numpy(), rtol=1e-5, atol=0.0)   # a dozen fp32 roundings per entry
        assert torch.equal(bnn.EdgeWeightNorm(norm, eps=eps)(g, w.view(-1, 1)), got)
    if norm != "none":
        assert not torch.equal(bnn.EdgeWeightNorm(norm, eps=0.5)(g, w), bnn.EdgeWeightNorm(norm)(g, w))
    if norm == "right":                                              # row-stochastic: the weights into a node sum to 1
        sums = torch.zeros(n, dtype=F64).index_add_(0, dst, bnn.EdgeWeightNorm(norm)(g, w).double())
        assert float((sums - 1).abs().max()) < 1e-5
    bad = w.clone()
    bad[7] = 0.0
    if norm == "both":
        with pytest.raises(DGLError, match="Non-positive"):
            bnn.EdgeWeightNorm(norm)(g, bad)
    else:
        bnn.EdgeWeightNorm(norm)(g, bad)
    with pytest.raises(DGLError):
        bnn.EdgeWeightNorm("left")
    with pytest.raises(DGLError):
        bnn.EdgeWeightNorm(norm)(g, w[:-1])
    assert "EdgeWeightNorm" in bnn.__all__


# ------------------------------------------------------------------------------------------------ 4. propagation on CPU tensors
@pytest.mark.parametrize("adj", ["DAD", "DA", "AD"])
@pytest.mark.parametrize("name", ["tiny", "small"])
def test_weighted_propagation_on_cpu_tensors_against_fp64_restatement(name, adj):
    """Weighted LP and C&S (50 + 50 iterations, alpha 0.8, weights uniform in [0.5, 1.5)) in the fp32 tensor form on CPU tensors against
    the float64 restatement: every entry within 1.0e-5 absolute.  Measured maxima over these cases: Correct and Smooth 5.3e-7
    ("small", DAD, fixed scale), label propagation 4.1e-7 ("small", AD); on "tiny" at most 1.6e-7."""
    src, dst, n = SC.graph(name)
    g = bot_amd.Graph(src, dst, n)
    w = EW.weights(name)
    assert float(w.min()) >= 0.5 and float(w.max()) < 1.5
    C = 7
    y_soft, y_true, mask = SC.cs_inputs(name, C)
    worst = 0.0
    for autoscale in (True, False):
        ref, raw = EW.cs_reference(name, C, adj, autoscale)
        assert SC.scale_margin(raw) > 0.01, "a raw autoscale factor lies within 1 % of the threshold: choose another seed"
        cs = smoothing.CorrectAndSmooth(correction_adj=adj, smoothing_adj=adj, autoscale=autoscale)
        got = cs(g, y_soft, y_true, mask, edge_weight=w)
        err = (got.double() - ref).abs().max().item()
        print(f"weighted C&S {name} {adj} autoscale={autoscale}: fp32 tensor form max |diff| = {err:.3e}")
        worst = max(worst, err)
        assert got.dtype == torch.float32 and err <= TOL
        plain = SC.cs_reference(name, C, adj, autoscale)[0]
        assert (ref - plain).abs().max().item() > 1e-3               # the weights change the result
    labels, ref = EW.lp_reference(name, C, adj)
    lp = smoothing.LabelPropagation(50, 0.8, adj)
    g.edata["w"] = w.view(-1, 1)
    got = lp(g, labels, mask=mask, edge_weight="w")                  # an edata key, [E, 1]
    err = (got.double() - ref).abs().max().item()
    print(f"weighted LP {name} {adj}: fp32 tensor form max |diff| = {err:.3e}; worst {max(worst, err):.3e}")
    assert err <= TOL
    assert torch.equal(lp(g, labels, mask=mask, edge_weight=w), got)


@pytest.mark.parametrize("adj", ["DAD", "DA", "AD"])
def test_unit_weights_give_the_unweighted_result_bit_for_bit(adj):
    src, dst, n = SC.graph("small")
    g = bot_amd.Graph(src, dst, n)
    y_soft, y_true, mask = SC.cs_inputs("small", 7)
    ones = torch.ones(src.numel())
    for autoscale in (True, False):
        cs = smoothing.CorrectAndSmooth(10, 0.8, adj, 10, 0.8, adj, autoscale=autoscale)
        assert torch.equal(cs(g, y_soft, y_true, mask, edge_weight=ones), cs(g, y_soft, y_true, mask))
        assert torch.equal(cs.smooth(g, cs.correct(g, y_soft, y_true, mask, ones), y_true, mask, ones), cs(g, y_soft, y_true, mask))
    ss, ds = smoothing._degree_scales(g, adj)
    ws, wd = smoothing._degree_scales(g, adj, smoothing._weights(g, ones))
    assert all(a is b or torch.equal(a, b) for a, b in ((ss, ws), (ds, wd)))


def test_weight_cache_follows_the_tensor_and_its_version():
    src, dst, n = SC.graph("tiny")
    g = bot_amd.Graph(src, dst, n)
    w = EW.weights("tiny").clone()
    y = torch.rand(n, 3, generator=torch.Generator().manual_seed(1))
    lp = smoothing.LabelPropagation(5, 0.7, "DA")
    a = lp(g, y, edge_weight=w)
    st = smoothing._weights(g, w)
    assert smoothing._weights(g, w) is st and "deg" in st              # prepared once
    w[::3] *= 4.0                                                       # in place: the version moves
    b = lp(g, y, edge_weight=w)
    assert smoothing._weights(g, w) is not st and not torch.equal(a, b)
    want = EW.label_propagation(src, dst, n, w, y, 5, 0.7, "DA")
    assert (b.double() - want).abs().max().item() <= TOL
    with pytest.raises(ValueError):
        lp(g, y, edge_weight=w[:-1])
    with pytest.raises(ValueError):
        lp(g, y, edge_weight=w.double())
    with pytest.raises(TypeError):
        lp(g, y, edge_weight=3.0)


def test_kernel_form_passes_the_weight_in_position_order(monkeypatch):
    """`impl="kernel"` on CPU tensors over the stand-in for the weighted `_C.propagate_step`: the weight arrives as `ew` in CSC position
    order on every sweep, and the run agrees with the restatement; without a weight the call carries no `ew`."""
    from bot_amd import _C
    seen = []

    def spy(*a, **kw):
        seen.append(kw.get("ew", "absent"))
        return EW.propagate_step_standin(*a, **kw)
    monkeypatch.setattr(_C, "propagate_step", spy)
    src, dst, n = SC.graph("tiny")
    g = bot_amd.Graph(src, dst, n)
    w = EW.weights("tiny")
    y = torch.rand(n, 5, generator=torch.Generator().manual_seed(2))
    for adj in ("DAD", "DA", "AD"):
        seen.clear()
        got = smoothing.propagate(g, y, 6, 0.8, adj, "clamp01", impl="kernel", want_abs=True, edge_weight=w)
        assert len(seen) == 6 and all(torch.equal(e, w[g.csc.eid.long()]) for e in seen)
        want = EW.propagate(src, dst, n, w, y, 6, 0.8, adj, "clamp01")
        assert (got[0].double() - want).abs().max().item() <= TOL
        assert (got[1].double() - want.abs().sum(1)).abs().max().item() <= 10 * TOL
    seen.clear()
    smoothing.propagate(g, y, 2, 0.8, "DAD", impl="kernel")
    assert seen == ["absent", "absent"]


# ------------------------------------------------------------------------------------------------ 5. saint_norms
@pytest.mark.parametrize("reordered", [False, True])
def test_saint_norms_bit_exact_against_the_restatement(backend, reordered):
    from bot_amd.sampling import SAINTSampler, saint_loss_weights, saint_norms
    g = _graph(n=600, e_raw=5000, seed=2)
    if reordered:
        g = reorder_graph(g, "degree")
    n, E = g.number_of_nodes(), g.number_of_edges()
    src, dst = (t.numpy() for t in g.edges())
    K = 30
    for sampler in (SAINTSampler("walk", (12, 2)), SAINTSampler("node", 60)):
        lw, en = saint_norms(g, sampler, K, seed=3)
        assert torch.equal(lw, saint_loss_weights(g, sampler, K, seed=3))              # bit for bit
        want_lw, want_en, sets, count, T = EW.saint_norms_reference(g, sampler, K, seed=3)
        assert np.array_equal(lw.numpy(), want_lw)
        assert en.dtype == torch.float32 and en.shape == (E,) and np.array_equal(en.numpy(), want_en)
        assert bool((torch.as_tensor(sampling._node_map(g)) == -1).all())
        # the consequences the docstring states
        assert float(en.min()) >= 1.0 and float(en.max()) <= K and int((T > 0).sum()) > 0 and int((T == 0).sum()) > 0
        assert np.all(T <= np.minimum(count[src], count[dst]))
        loops = src == dst
        assert loops.sum() == n and np.all(want_en[loops] == 1.0) and np.all(T[loops] == count[dst[loops]])
        assert np.all(want_en[T == 0] == 1.0)
        # the identity the norm exists for, in float64: for v with C[v] > 0 the mean over the sets that hold v of the weighted sum over
        # the in-edges the set induces equals the sum over the in-edges ever induced
        x = np.random.default_rng(1).standard_normal(n)
        norm64 = np.where(T > 0, count[dst] / np.maximum(T, 1), 1.0)
        acc = np.zeros(n)
        for s in sets:
            member = np.zeros(n, dtype=bool)
            member[s] = True
            m = member[src] & member[dst]
            np.add.at(acc, dst[m], norm64[m] * x[src[m]])
        want = np.zeros(n)
        np.add.at(want, dst[T > 0], x[src[T > 0]])
        scale = np.zeros(n)
        np.add.at(scale, dst[T > 0], np.abs(x[src[T > 0]]))
        seen = count > 0
        assert seen.sum() > 0 and np.all(np.abs(acc[seen] / count[seen] - want[seen]) <= 1e-12 * scale[seen])
        assert not np.any(acc[~seen])
    with pytest.raises(ValueError):
        saint_norms(g, SAINTSampler("node", 60), 2 ** 24)
    with pytest.raises(ValueError):
        saint_norms(g, SAINTSampler("node", 60), 0)


def test_tally_restatement_counts_induced_edges():
    g = _graph(n=80, e_raw=400, seed=9)
    indptr, indices, eid = SGC.csc_arrays(g)
    rng = np.random.default_rng(0)
    sets = [rng.permutation(80)[:k] for k in (0, 1, 30, 80)]
    T = EW.tally_reference(indptr, indices, sets)
    for k, s in zip((0, 1, 30, 80), sets):
        one = EW.tally_reference(indptr, indices, [s])
        _, _, pe = SGC.induced_reference(indptr, indices, eid, s)
        kept = np.zeros(len(indices), dtype=np.int32)
        kept[np.argsort(eid)[pe]] = 1                               # parent edge id -> its CSC position
        assert np.array_equal(one, kept) and one.sum() == len(pe)
    assert np.array_equal(T, sum(EW.tally_reference(indptr, indices, [s]) for s in sets))
    assert np.all(EW.tally_reference(indptr, indices, [sets[3]]) == 1)


# ------------------------------------------------------------------------------------------------ 6. through the step
def test_build_saint_aggregator_norm_on_the_emulated_backend(backend, monkeypatch):
    from bot_amd import _C, minibatch, workloads
    from bot_amd import train as T
    from tests.test_saint_host import node_loss_weighted_standin
    monkeypatch.setattr(_C, "node_loss_weighted", node_loss_weighted_standin)
    wl = workloads.build_saint("cora", "cpu", scale=0.3, aggregator_norm=True)
    g = wl.graph
    assert wl.edge_weight == "saint_norm" == workloads.SAINT_NORM and "aggregator" in wl.describe
    en = g.edata["saint_norm"]
    assert en.shape == (g.number_of_edges(),) and en.dtype == torch.float32 and float(en.min()) >= 1.0 and float(en.max()) > 1.0
    plain = workloads.build_saint("cora", "cpu", scale=0.3)
    assert plain.edge_weight is None and "saint_norm" not in plain.graph.edata and torch.equal(plain.loss_weight, wl.loss_weight)
    assert plain.step_kw == wl.step_kw and "edge_weight" not in plain.step_kw
    assert type(plain.loader) is type(wl.loader) and plain.loader.n_batches == wl.loader.n_batches
    assert plain.loader.sampler.budget == wl.loader.sampler.budget
    # the batch's rows of the column reach the model
    seen = []
    real = T.train_step

    def spy(model, graph, feat, *a, **kw):
        seen.append((graph, kw.get("edge_weight")))
        return real(model, graph, feat, *a, **kw)
    monkeypatch.setattr(T, "train_step", spy)
    loss, skipped = wl.epoch()
    assert math.isfinite(loss) and len(seen) + skipped == len(wl.loader)
    assert all(w is not None and torch.equal(w, en[sub.parent_eid.long()]) for sub, w in seen)
    seen.clear()
    loss, _ = plain.epoch()
    assert math.isfinite(loss) and seen and all(w is None for _, w in seen)
    for name in ("arxiv", "products", "proteins"):
        with pytest.raises(ValueError, match="GCN"):
            workloads.build_saint(name, "cpu", scale=0.01, aggregator_norm=True)
    # a GAT stack or an edge-feature stack refuses a weight
    sub = next(iter(wl.loader))
    gat = bnn.GAT(dim_node=4, dim_edge=0, dim_output=3, n_hidden=4, n_layers=2, n_heads=1, activation=F.relu)
    with pytest.raises(ValueError, match="GCN"):
        minibatch.subgraph_step(gat, sub, None, wl.labels, wl.roles, step_kw={}, edge_weight="saint_norm")
    with pytest.raises(ValueError, match="GCN"):
        minibatch.subgraph_step(wl.model, sub, None, wl.labels, wl.roles, node_loss=lambda x, y: x, edge_weight="saint_norm")


def test_train_step_calls_the_model_with_a_weight_only_when_given(backend, monkeypatch):
    from bot_amd import train as T
    g = _graph()
    n, E = g.number_of_nodes(), g.number_of_edges()
    gen = torch.Generator().manual_seed(1)
    feat, labels = torch.randn(n, 6, generator=gen), torch.randint(0, 4, (n, 1), generator=gen)
    tr = torch.arange(0, n, 2)
    w = 0.5 + torch.rand(E, generator=gen)
    calls = []

    class Probe(bnn.GCN):
        def forward(self, *a, **kw):
            calls.append((len(a), sorted(kw)))
            return super().forward(*a, **kw)
    for fused_step in (True, False):
        monkeypatch.setattr(T, "FUSED_STEP", fused_step)
        torch.manual_seed(0)
        model = Probe(in_feats=6, n_classes=4, n_hidden=8, n_layers=2, activation=F.relu, norm="none", norm_adj="symm")
        opt = torch.optim.SGD(model.parameters(), lr=0.0)
        kw = dict(use_labels=False, loss="logit", n_classes=4, mask=torch.rand(tr.shape, generator=gen) < 0.5)
        calls.clear()
        l0, _ = T.train_step(model, g, feat, labels, tr, None, None, opt, **kw)
        assert calls == [(2, [])]                                    # today's call
        calls.clear()
        l1, _ = T.train_step(model, g, feat, labels, tr, None, None, opt, edge_weight=w, **kw)
        assert calls == [(2, ["edge_weight"])]
        l2, _ = T.train_step(model, g, feat, labels, tr, None, None, opt, edge_weight=torch.ones(E), **kw)
        l0, l1, l2 = (float(x.detach()) for x in (l0, l1, l2))
        assert abs(l2 - l0) <= 2e-6 * max(1.0, abs(l0)) and abs(l1 - l0) > 1e-6


# ------------------------------------------------------------------------------------------------ 7. symbols
def test_edge_weight_symbols_are_exported_and_validate_arguments():
    from bot_amd import _C
    lib = _C._lib
    for name in ("bot_propagate_step_w_f32", "bot_subgraph_tally_i32"):
        assert name in _C.EXPORTED and hasattr(lib, name)
    assert "bot_propagate_step_f32" in _C.EXPORTED and lib.bot_abi_version() == 19 == _C.ABI_VERSION
    ibuf = (ctypes.c_int32 * 16)()
    p = ctypes.addressof(ibuf)
    tally = lib.bot_subgraph_tally_i32
    assert tally(None, p, 4, p, 2, p, p, None) == -1 and b"subgraph_tally" in lib.bot_last_error()
    assert tally(p, p, 4, p, 2, None, p, None) == -1
    assert tally(p, None, 4, p, 2, p, p, None) == -1
    assert tally(p, p, 4, None, 2, p, p, None) == -1
    assert tally(p, p, 4, p, 2, p, None, None) == -1
    assert tally(p, p, -4, p, 2, p, p, None) == -2 and tally(p, p, 4, p, -2, p, p, None) == -2 and tally(p, p, 4, p, 5, p, p, None) == -2
    assert tally(p, None, 4, None, 0, p, None, None) == 0             # no nodes: nothing launched
    buf = (ctypes.c_float * 64)()
    items = (ctypes.c_int32 * 64)()
    f, f2 = ctypes.addressof(buf), ctypes.addressof(buf) + 128
    it = (ctypes.addressof(items) + 15) // 16 * 16

    def call(y=f, y0=f, out=f2, C=4, n=4, nnz=0, items=it, ld=4, n_long=0, ew=f):
        return lib.bot_propagate_step_w_f32(None, None, n, nnz, items, n, None, None, n_long, y, ld, y0, ld, out, ld, C, 0.5, 0.5, None, None,
                                            -math.inf, math.inf, None, None, None, None, ew, None)
    assert call(y=None) == -1 and b"NULL" in lib.bot_last_error()
    assert call(y0=None) == -1 and call(out=None) == -1 and call(items=None) == -1 and call(nnz=3) == -1 and call(n_long=1) == -1
    assert call(C=0) == -2 and call(C=1025, ld=1025) == -2 and call(n=-1) == -2 and call(ld=3) == -2
    assert call(out=f) == -2 and b"alias" in lib.bot_last_error()
    assert call(ew=f + 2) == -3 and b"misaligned" in lib.bot_last_error()
    assert call(y=None, y0=None, out=None, items=None, n=0) == 0 and call(y=None, y0=None, out=None, items=None, n=0, ew=None) == 0
    assert call(y=None, ew=None) == -1                               # a NULL weight: the unweighted entry's checks
    # the wrappers refuse CPU tensors: there is no fallback
    g = _graph(n=50, e_raw=300, seed=5)
    with pytest.raises(_C.BotKernelError):
        _C.subgraph_tally(g.csc, torch.arange(4, dtype=torch.int32), torch.full((50,), -1, dtype=torch.int32),
                          torch.zeros(g.number_of_edges(), dtype=torch.int32))
    y = torch.zeros(50, 3)
    with pytest.raises(_C.BotKernelError):
        _C.propagate_step(g.csc, y, y.clone(), y.clone(), 0.5, 0.5, None, None, 0.0, 1.0, ew=torch.ones(g.number_of_edges()))
