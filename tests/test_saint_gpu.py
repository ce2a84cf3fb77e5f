"""GraphSAINT batches on the MI355X: the walk kernel (csrc/saint.hip) and the node list (csrc/sampling.hip) against the numpy
restatement (tests/saint_cases.py) bit for bit, the weighted loss kernel (csrc/step.hip) against the float64 tensor-op form, one
weighted train step of the GAT / GCN / ProductsGAT stacks on a SAINT batch against the float64 oracle (constants of
tests/parity_cases.py), unit weights against the unweighted fused step bit for bit, and three SAINT epochs of S-arxiv."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bot_amd
from bot_amd import _C, minibatch, synth
from bot_amd import nn as bnn
from bot_amd import train as T
from bot_amd.nn import fused
from bot_amd.sampling import SAINTSampler, _node_map, node_subgraph
from oracle import ref_models as RM
from tests import parity_cases as PC
from tests import saint_cases as SN
from tests import subgraph_cases as SC
from tests.test_subgraph_gpu import _f64, _hub_graph, _parent

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _holed_hub_graph():
    """The hub graph's raw edges without the in-edges of every seventh node: nodes with no in-edge, where a walk stays."""
    n = 30000
    rs, rd = synth.powerlaw_edges(n, 1500000, 11)
    keep = (rd % 7) != 0
    return bot_amd.Graph(rs[keep], rd[keep], n).remove_self_loop().to(DEV)


# ------------------------------------------------------------------------------------------------ 1. the walks
@pytest.mark.parametrize("kind", ["loops", "raw", "holed"])
def test_walks_against_the_restatement_bit_for_bit(kind):
    """The hub graph of tests/test_subgraph_gpu.py preprocessed ("loops") and as raw directed edges ("raw"), R in {1, 63, 64, 65, 5000},
    L in {0, 1, 2, 5}, both root modes, nids given and NULL, two seeds; two calls give identical bytes.  The raw hub graph turned out
    to have no node without in-edges (1.5 M edges over 30 000 nodes), so the stay-where-you-are branch is held on a third graph,
    "holed": the same edges without the in-edges of every seventh node; there a walk must meet such a node."""
    g = _hub_graph(loops=True) if kind == "loops" else (_hub_graph(loops=False) if kind == "raw" else _holed_hub_graph())
    indptr, indices, _ = SC.csc_arrays(g)
    n = g.number_of_nodes()
    deg = np.diff(indptr)
    assert deg.max() > 2048
    if kind == "holed":
        assert (deg == 0).sum() >= n // 7
    elif kind == "raw":
        assert (deg == 0).sum() == 0                                            # why the third graph exists
    nids_np = np.random.default_rng(3).permutation(n)[:777].astype(np.int32)
    nids = torch.from_numpy(nids_np).to(DEV)
    stayed = 0
    for R in (1, 63, 64, 65, 5000):
        for L in (0, 1, 2, 5):
            for root_mode, ids, ids_np in ((0, None, None), (0, nids, nids_np), (1, None, None)):
                for seed in (7, -(2 ** 62) - 12345):
                    got = _C.saint_walk(g.csc, ids, R, L, root_mode, seed)
                    assert got.shape == (R, L + 1) and got.dtype == torch.int32
                    a = got.cpu().numpy()
                    want = SN.walk_reference(indptr, indices, ids_np, R, L, root_mode, seed)
                    assert np.array_equal(a, want), (kind, R, L, root_mode, ids is not None, seed)
                    again = _C.saint_walk(g.csc, ids, R, L, root_mode, seed).cpu().numpy()
                    assert a.tobytes() == again.tobytes()
                    if L:
                        stayed += int((deg[a[:, :-1]] == 0).sum())
    assert stayed > 0 or kind != "holed"                                        # a walk met a node without in-edges and stayed
    assert _C.saint_walk(g.csc, None, 0, 3, 0, 1).shape == (0, 4)


# ------------------------------------------------------------------------------------------------ 2. the node list
def test_node_list_is_the_ascending_set_and_leaves_the_map_clean():
    g = _hub_graph()
    indptr, indices, _ = SC.csc_arrays(g)
    m = _node_map(g)
    for R, L, root_mode in ((1, 0, 0), (64, 2, 0), (5000, 2, 0), (5000, 5, 1), (20000, 0, 1), (70000, 1, 0)):
        trace = _C.saint_walk(g.csc, None, R, L, root_mode, 5)
        nodes = _C.saint_nodes(trace, m)
        want = SN.node_set_reference(SN.walk_reference(indptr, indices, None, R, L, root_mode, 5))
        got = nodes.cpu().numpy()
        assert nodes.dtype == torch.int32 and np.array_equal(got, want)
        assert np.all(np.diff(got) > 0)                                                          # ascending, duplicate-free
        assert bool((m == -1).all())
        assert torch.equal(nodes, _C.saint_nodes(trace, m))
    empty = _C.saint_nodes(_C.saint_walk(g.csc, None, 0, 2, 0, 1), m)
    assert empty.numel() == 0 and empty.dtype == torch.int32 and bool((m == -1).all())
    # ids outside the graph are skipped and reported; the map is left clean and serves the next call
    bad = torch.tensor([[5, -1, 9], [g.number_of_nodes(), 5, 2 ** 31 - 1]], dtype=torch.int32, device=DEV)
    with pytest.raises(ValueError, match="3 entries"):
        _C.saint_nodes(bad, m)
    assert bool((m == -1).all())
    assert _C.saint_nodes(torch.tensor([9, 5, 9], dtype=torch.int32, device=DEV), m).tolist() == [5, 9]


# ------------------------------------------------------------------------------------------------ 3. the sampler
@pytest.mark.parametrize("reorder", [None, "degree"])
def test_sampler_batches_are_the_induced_subgraphs_of_the_restated_node_sets(reorder):
    rs, rd = synth.powerlaw_edges(6000, 60000, 7)
    g = bot_amd.preprocess(bot_amd.Graph(rs, rd, 6000).to(DEV), reorder=reorder)
    samplers = (SAINTSampler("walk", (70, 2)), SAINTSampler("node", 200), SAINTSampler("walk", (50, 3), nids=torch.arange(0, 6000, 5)))
    for sampler in samplers:
        for seed in (0, 123456789):
            want_nodes = SN.sampler_nodes_reference(g, sampler, seed)
            nodes = sampler.sample_nodes(g, seed)
            assert np.array_equal(nodes.cpu().numpy(), want_nodes)
            sub = sampler.sample(g, seed)
            ref = node_subgraph(g, torch.from_numpy(want_nodes))
            assert torch.equal(sub.parent_nid, ref.parent_nid) and torch.equal(sub.parent_eid, ref.parent_eid)
            assert torch.equal(sub.csc.indptr, ref.csc.indptr) and torch.equal(sub.csc.indices, ref.csc.indices)
            assert torch.equal(sub.parent_rows, ref.parent_rows)
            off, src, pe = SC.induced_reference(*SC.csc_arrays(g), want_nodes)
            assert np.array_equal(sub.csc.indices.cpu().numpy(), src) and np.array_equal(sub.parent_eid.cpu().numpy(), pe)
    # the loss weights on the device equal the restatement
    from bot_amd.sampling import saint_loss_weights
    lw = saint_loss_weights(g, samplers[0], 20, seed=1)
    want, _, _ = SN.loss_weights_reference(g, samplers[0], 20, seed=1)
    assert lw.is_cuda and np.array_equal(lw.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ 4. the weighted loss kernel
@pytest.mark.parametrize("C", [7, 40, 128])
@pytest.mark.parametrize("kind", ["logit", "loge", "savage"])
def test_weighted_loss_kernel_against_the_float64_form(kind, C):
    n = 1003
    gen = torch.Generator().manual_seed(C)
    pred = 2 * torch.randn(n, C, generator=gen)
    labels = torch.randint(0, C, (n, 1), generator=gen)
    wn = (torch.rand(n, generator=gen) < 0.4).float()
    labels[wn == 0] = -1                                                                         # placeholders
    lw = 0.5 + 3.5 * torch.rand(n, generator=gen)
    on = wn > 0
    wsum = lw[on].double().sum().float().reshape(1)
    y, dx = _C.node_loss_weighted(pred.to(DEV), labels.to(DEV), wn.to(DEV), lw.to(DEV), wsum.to(DEV), kind, T.EPSILON)
    assert y.shape == (1024,) and dx.shape == (n, C)
    y, dx = y.cpu(), dx.cpu()
    p64 = pred.double().requires_grad_()
    per = T.per_node_loss(p64, labels.clamp(0, C - 1), kind)
    y64 = torch.where(on, lw.double() * per, torch.zeros_like(per)).detach()
    loss64 = T.weighted_node_loss(p64, labels, wn, lw.double(), kind)
    (dx64,) = torch.autograd.grad(loss64, p64)
    # the kernel divides by the fp32 wsum it is handed; the float64 form by its own sum: the same number to 1e-7
    ey = float((y[:n].double() - y64).abs().max()) / float(y64.abs().max())
    ed = float((dx.double() - dx64).abs().max()) / float(dx64.abs().max())
    print(kind, C, "y", ey, "dx", ed)
    assert ey <= PC.GRAD_RTOL and ed <= PC.GRAD_RTOL
    assert not y[:n][~on].any() and not y[n:].any() and not dx[~on].any()                        # exact zeros
    assert abs(float(y.double().sum() / wsum.double()) - float(loss64)) <= PC.GRAD_RTOL * abs(float(loss64))
    # lw = 1 and wsum = count: node_loss's bits
    count = wn.sum().reshape(1)
    args = (pred.to(DEV), labels.to(DEV), wn.to(DEV))
    y1, dx1 = _C.node_loss_weighted(*args, torch.ones(n, device=DEV), count.to(DEV), kind, T.EPSILON)
    y0, dx0 = _C.node_loss(*args, count.to(DEV), kind, T.EPSILON)
    assert torch.equal(y1, y0) and torch.equal(dx1, dx0)
    y2, dx2 = _C.node_loss_weighted(*args, torch.ones(n, device=DEV), count.to(DEV), kind, T.EPSILON, want_grad=False)
    assert dx2 is None and torch.equal(y2, y0)


# ------------------------------------------------------------------------------------------------ 5. the weighted step against the oracle
def _saint_batch(g, seed=4):
    sub = SAINTSampler("walk", (700, 2)).sample(g, seed)
    n = sub.number_of_nodes()
    assert 1000 < n < 2101
    gen = torch.Generator().manual_seed(seed)
    lw = 0.5 + 3.5 * torch.rand(g.number_of_nodes(), generator=gen)
    return sub, n, lw, gen


def _oracle_grads(ref, loss64, sd, model, pred, names=None):
    loss64.backward()
    PC.fwd_close(pred, ref.detach().numpy())
    checked = 0
    for k, p in model.named_parameters():
        if sd[k].grad is None:
            assert p.grad is None or not p.grad.any(), k
            continue
        PC.grad_close(p.grad, sd[k].grad.numpy())
        checked += 1
    assert checked >= 6
    print("worst gradient error / largest entry", max(PC.WORST[-checked:]))


@pytest.mark.parametrize("stack", ["gat", "gcn"])
@pytest.mark.parametrize("kind", ["loge", "logit"])
def test_weighted_train_step_on_a_saint_batch_against_the_oracle(stack, kind):
    g = _parent()
    sub, n, lw_parent, gen = _saint_batch(g)
    C = 7
    torch.manual_seed(0)
    if stack == "gat":
        cfg = dict(n_layers=3, n_heads=3, n_hidden=32, norm="batch", non_interactive_attn=True, use_symmetric_norm=False, linear=True,
                   residual=False)
        model = bnn.GAT(dim_node=24, dim_edge=0, dim_output=C, activation=F.relu, **cfg).to(DEV).train()
    else:
        model = bnn.GCN(in_feats=24, n_classes=C, n_hidden=32, n_layers=3, activation=F.relu, norm="batch", norm_adj="symm",
                        dropout=0.0).to(DEV).train()
    feat = sub.ndata["feat"]
    labels = torch.randint(0, C, (n, 1), generator=gen)
    perm = torch.randperm(n, generator=gen)
    tr = perm[: n // 2].to(DEV)
    mask = torch.rand(n // 2, generator=gen) < 0.5
    lw = lw_parent.to(DEV)[sub.parent_rows]                                                      # the batch's slice
    sd = _f64(model)
    model.zero_grad(set_to_none=True)
    c0 = fused.CALLS
    loss, pred, wn = T.forward_backward(model, sub, feat, labels.to(DEV), tr, None, None, use_labels=False, loss=kind, n_classes=C,
                                        mask=mask.to(DEV), loss_weight=lw)
    assert (fused.CALLS > c0 or stack != "gat") and wn.shape == (n,)                             # the fused full-batch layers ran on the batch
    s, d = (t.cpu() for t in sub.edges())
    if stack == "gat":
        ref = RM.gat_forward(RM.CooGraph(s, d, n), feat.cpu().double(), sd, n_classes=C, training=True, **cfg)
    else:
        ref = RM.gcn_forward(RM.CooGraph(s, d, n), feat.cpu().double(), sd, n_layers=3, norm="batch", norm_adj="symm", training=True)
    wn64 = torch.zeros(n)
    wn64[tr.cpu()] = mask.float()                                                                # use_labels off: the masked-in nodes predict
    assert torch.equal(wn.cpu(), wn64)
    loss64 = SN.weighted_loss_formula(ref, labels, wn64, lw.cpu().double(), kind, T.EPSILON)
    print("loss", float(loss.detach()), float(loss64.detach()))
    assert abs(float(loss.detach()) - float(loss64.detach())) <= PC.FWD_ATOL
    _oracle_grads(ref, loss64, sd, model, pred)


def test_weighted_products_gat_step_on_a_saint_batch_against_the_oracle():
    from bot_amd.nn import edge_gat
    g = _parent()
    sub, n, lw_parent, gen = _saint_batch(g)
    C = 12
    torch.manual_seed(8)
    model = edge_gat.ProductsGAT(node_feats=24, edge_feats=0, n_classes=C, n_layers=3, n_heads=4, n_hidden=20, edge_emb=0,
                                 activation=F.relu, dropout=0.0, input_drop=0.0, attn_drop=0.0, edge_drop=0.0).to(DEV).train()
    N = g.number_of_nodes()
    labels = torch.randint(0, C, (N, 1), generator=gen).to(DEV)                                  # the parent's, original order
    train_idx = torch.randperm(N, generator=gen)[: N // 2].to(DEV)
    roles = minibatch.node_roles(N, train_idx)
    lw = lw_parent.to(DEV)

    def loge(x, y):
        ce = F.cross_entropy(x, y[:, 0], reduction="none")
        return torch.log(T.EPSILON + ce) - math.log(T.EPSILON)
    sd = _f64(model)
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    loss, pred, n_tr = minibatch.subgraph_step(model, sub, opt, labels, roles, node_loss=loge, loss_weight=lw)
    rows = sub.parent_rows
    assert n_tr == int((roles[rows] == 1).sum()) and 0 < n_tr < n
    s, d = (t.cpu() for t in sub.edges())
    ref = RM.proteins_gat_forward(RM.CooGraph(s, d, n), sub.ndata["feat"].cpu().double(), None, sd, n_layers=3, n_heads=4, n_hidden=20,
                                  training=True, use_node_encoder=False, residual=False)
    wn64 = (roles[rows] == 1).float().cpu()
    loss64 = SN.weighted_loss_formula(ref, labels[rows].cpu(), wn64, lw[rows].cpu().double(), "loge", T.EPSILON)
    assert abs(float(loss.detach()) - float(loss64.detach())) <= PC.FWD_ATOL
    _oracle_grads(ref, loss64, sd, model, pred)
    plain = minibatch.subgraph_step(model, sub, opt, labels, roles, node_loss=loge)
    assert abs(float(plain[0].detach()) - float(loss.detach())) > 1e-6                           # the weights reach the loss


# ------------------------------------------------------------------------------------------------ 6. unit weights: the unweighted step's bits
@pytest.mark.parametrize("use_labels", [False, True])
def test_unit_weights_give_the_unweighted_fused_step_bit_for_bit(use_labels):
    g = _parent()
    sub, n, _, gen = _saint_batch(g)
    C = 7
    cfg = dict(n_layers=3, n_heads=3, n_hidden=32, norm="batch", non_interactive_attn=True, use_symmetric_norm=False, linear=True,
               residual=False, dropout=0.0, input_drop=0.0, attn_drop=0.0, edge_drop=0.0)
    torch.manual_seed(0)
    model = bnn.GAT(dim_node=24 + (C if use_labels else 0), dim_edge=0, dim_output=C, activation=F.relu, **cfg).to(DEV).train()
    state = {k: v.clone() for k, v in model.state_dict().items()}
    feat = sub.ndata["feat"]
    labels = torch.randint(0, C, (n, 1), generator=gen).to(DEV)
    tr = torch.randperm(n, generator=gen)[: n // 2].to(DEV)
    mask = (torch.rand(n // 2, generator=gen) < 0.5).to(DEV)
    kw = dict(use_labels=use_labels, loss="loge", n_classes=C, mask=mask)

    def run(loss_weight):
        model.load_state_dict(state)
        model.zero_grad(set_to_none=True)
        loss, pred, _ = T.forward_backward(model, sub, feat, labels, tr, None, None, loss_weight=loss_weight, **kw)
        return loss.detach().clone(), pred.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    assert T.FUSED_STEP
    l0, p0, g0 = run(None)
    l1, p1, g1 = run(torch.ones(n, device=DEV))
    assert torch.equal(l0, l1) and torch.equal(p0, p1) and g0.keys() == g1.keys() and len(g0) >= 6
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    l2, _, g2 = run(0.5 + torch.rand(n, generator=gen).to(DEV))
    assert not torch.equal(l0, l2) and any(not torch.equal(g0[k], g2[k]) for k in g0)


# ------------------------------------------------------------------------------------------------ 7. epochs
def test_three_saint_epochs_of_arxiv(monkeypatch):
    """S-arxiv at scale 0.05 (the scale of the clustered epochs' test): finite losses, no skipped batch, and every batch holds at
    least 2 (n - r) edges that are not self-loops (n nodes, r distinct roots: the bound of the host suite's structure test)."""
    from bot_amd import workloads
    torch.manual_seed(0)
    wl = workloads.build_saint("arxiv", DEV, scale=0.05, seed=0, drop=False)
    N = wl.graph.number_of_nodes()
    assert len(wl.loader) == 30 and wl.step_kw["use_labels"] and wl.loss_weight.shape == (N,)
    assert wl.loader.sampler.n_roots == math.ceil(N / 90) and wl.loader.sampler.length == 2
    assert float(wl.loss_weight.min()) >= 1.0 and float(wl.loss_weight.max()) <= 1500.0
    roots, batches = [], []
    walk, step = _C.saint_walk, minibatch.subgraph_step

    def spy_walk(*a, **k):
        trace = walk(*a, **k)
        roots.append(int(torch.unique(trace[:, 0]).numel()))
        return trace

    def spy_step(model, sub, *a, **k):
        s, d = sub.edges()
        batches.append((sub.number_of_nodes(), int((s != d).sum())))
        assert "loss_weight" in k and k["loss_weight"] is wl.loss_weight
        return step(model, sub, *a, **k)
    monkeypatch.setattr(_C, "saint_walk", spy_walk)
    monkeypatch.setattr(minibatch, "subgraph_step", spy_step)
    c0 = fused.CALLS
    out = [wl.epoch() for _ in range(3)]
    losses = [v for v, _ in out]
    print("losses", losses, "skipped", [s for _, s in out], "nodes per batch", sorted(n for n, _ in batches)[::30])
    assert all(math.isfinite(v) for v in losses) and all(s == 0 for _, s in out)
    assert fused.CALLS - c0 >= 3 * 30 and len(batches) == len(roots) == 90
    for (n, non_loop), r in zip(batches, roots):
        assert n <= 3 * wl.loader.sampler.n_roots and non_loop >= 2 * (n - r), (n, non_loop, r)
