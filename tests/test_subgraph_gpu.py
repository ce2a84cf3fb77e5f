"""Induced-subgraph (cluster) batches on the MI355X: the extraction kernels (csrc/subgraph.hip) against the numpy restatement
(tests/subgraph_cases.py) bit for bit, one train step of the GAT / GCN / ProductsGAT stacks on a `Subgraph` against the same step
on a `Graph` built from the subgraph's edge list and against the float64 oracle (constants of tests/parity_cases.py), the
all-parts-in-one-batch epoch against the full-batch step, and three clustered epochs of S-arxiv."""
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
from bot_amd.sampling import ClusterLoader, Subgraph, _node_map, cluster_assignment, node_subgraph
from oracle import ref_models as RM
from tests import parity_cases as PC
from tests import subgraph_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _hub_graph(loops=True):
    """Power-law graph whose hub row is longer than the plan chunk and than two steps of the long-row sweep."""
    n = 30000
    rs, rd = synth.powerlaw_edges(n, 1500000, 11)
    g = bot_amd.Graph(rs, rd, n)
    g = bot_amd.preprocess(g) if loops else g.remove_self_loop()
    return g.to(DEV)


def _extract(g, nodes):
    nodes = torch.as_tensor(nodes).to(DEV, torch.int32).contiguous()
    return tuple(t.cpu().numpy() for t in _C.node_subgraph(g.csc, nodes, _node_map(g)))


def _check_against_restatement(g, nodes):
    got = _extract(g, nodes)
    want = SC.induced_reference(*SC.csc_arrays(g), np.asarray(nodes))
    for a, b, what in zip(got, want, ("offsets", "local_src", "parent_eid")):
        assert a.dtype == b.dtype and np.array_equal(a, b), what
    assert bool((_node_map(g) == -1).all())
    again = _extract(g, nodes)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))             # two calls give identical bytes
    return got


def test_extraction_against_the_restatement_bit_for_bit():
    g = _hub_graph()
    n = g.number_of_nodes()
    indptr, indices, eid = SC.csc_arrays(g)
    deg = np.diff(indptr)
    assert deg.max() > 2 * SC.LONG_TILE and deg.max() > g.csc.chunk and g.csc.n_long > 0
    assert (deg > SC.LONG_ROW).sum() >= 3 and (deg <= SC.LONG_ROW).sum() > n // 2
    rng = np.random.default_rng(5)
    hubs = np.argsort(-deg)[:3]
    # empty
    off, src, pe = _check_against_restatement(g, np.zeros(0, dtype=np.int64))
    assert off.tolist() == [0] and len(src) == 0 and len(pe) == 0
    # a single node: its self-loop
    off, src, pe = _check_against_restatement(g, np.array([int(hubs[0])]))
    assert off.tolist() == [0, 1] and src.tolist() == [0]
    # every node in identity order: the parent's CSC
    off, src, pe = _check_against_restatement(g, np.arange(n))
    assert np.array_equal(off, indptr) and np.array_equal(src, indices) and np.array_equal(pe, eid)
    # every node, permuted
    _check_against_restatement(g, rng.permutation(n))
    # a random 1/30, once with the hubs forced in (long rows that keep a part of their edges), unsorted and sorted
    pick = rng.permutation(n)[:n // 30]
    _check_against_restatement(g, pick)
    with_hubs = np.unique(np.concatenate([pick, hubs]))
    off, _, _ = _check_against_restatement(g, with_hubs)
    kept = np.diff(off)[np.searchsorted(with_hubs, hubs)]
    assert np.all(kept > 64) and np.all(kept < deg[hubs])
    _check_against_restatement(g, rng.permutation(with_hubs))
    # half of the nodes: the hubs keep more than one step of the sweep
    half = np.unique(np.concatenate([hubs, rng.permutation(n)[:n // 2]]))
    off, _, _ = _check_against_restatement(g, half)
    assert np.diff(off)[np.searchsorted(half, hubs[0])] > SC.LONG_TILE


def test_extraction_where_rows_keep_nothing():
    g = _hub_graph(loops=False)                       # raw directed edges (parallel ones included), no self-loops
    n = g.number_of_nodes()
    rng = np.random.default_rng(6)
    for nodes in (rng.permutation(n)[:n // 30], np.arange(n), np.array([7])):
        off, src, pe = _check_against_restatement(g, nodes)
    off, _, _ = _check_against_restatement(g, rng.permutation(n)[:n // 30])
    assert (np.diff(off) == 0).sum() > 0 and off[-1] > 0


def test_duplicates_and_ids_out_of_range_raise_and_leave_the_map_clean():
    g = _hub_graph()
    n = g.number_of_nodes()
    m = _node_map(g)
    for bad in ([5, 9, 5], [3, 3, 3, 4], list(range(2000)) + [1999], [0, n], [-1, 2], [n + 5, n + 5]):
        with pytest.raises(ValueError):
            _C.node_subgraph(g.csc, torch.tensor(bad, dtype=torch.int32, device=DEV), m)
        assert bool((m == -1).all())
    with pytest.raises(ValueError):
        node_subgraph(g, torch.tensor([5, 9, 5], device=DEV))                       # device ids: the kernel's duplicate count
    with pytest.raises(ValueError):
        g.subgraph([5, 9, 5])                                                       # host ids: checked before the upload
    assert bool((m == -1).all())
    sub = g.subgraph(torch.tensor([5, 9, 7], device=DEV))                           # and the map still serves the next call
    assert isinstance(sub, Subgraph) and sub.parent_nid.tolist() == [5, 9, 7] and bool((m == -1).all())
    # the sampler shares the map
    from bot_amd.sampling import sample_block
    b = sample_block(g, torch.tensor([1, 2, 3], dtype=torch.int32, device=DEV), 4, 1)
    assert b.number_of_dst_nodes() == 3 and bool((m == -1).all())


# ------------------------------------------------------------------------------------------------ model parity
def _parent(n=6000, e_raw=60000, fin=24, seed=7):
    rs, rd = synth.powerlaw_edges(n, e_raw, seed)
    g = bot_amd.preprocess(bot_amd.Graph(rs, rd, n).to(DEV))
    g.ndata["feat"] = torch.randn(n, fin, generator=torch.Generator().manual_seed(seed + 1)).to(DEV)
    return g


def _sub_and_twin(g, n_sub=3000):
    nodes = torch.randperm(g.number_of_nodes(), generator=torch.Generator().manual_seed(2))[:n_sub].to(DEV)
    sub = g.subgraph(nodes)
    s, d = sub.edges()
    twin = bot_amd.graph((s.clone(), d.clone()), num_nodes=n_sub)                   # the parent commit's path to the same graph
    assert torch.equal(twin.csc.indptr, sub.csc.indptr) and torch.equal(twin.csc.indices, sub.csc.indices)
    assert torch.equal(twin.csc.eid, sub.csc.eid) and torch.equal(twin.csr.indptr, sub.csr.indptr)
    return sub, twin


def _f64(model):
    params = {k for k, _ in model.named_parameters()}
    return {k: (v.detach().cpu().double().requires_grad_(k in params) if v.is_floating_point() else v.cpu())
            for k, v in model.state_dict().items()}


def _step(model, run, gout):
    model.zero_grad(set_to_none=True)
    logits = run()
    (logits * gout).sum().backward()
    return logits.detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


def _compare(model, on_sub, on_twin, oracle_logits, sd, gout64):
    """Subgraph = twin Graph bit for bit on the logits (equal CSC contents, no float atomics); both within the suite's constants
    of the float64 oracle; the two GPU runs' gradients within the same constant of each other."""
    (ls, gs), (lt, gt) = on_sub, on_twin
    assert torch.equal(ls, lt), float((ls - lt).abs().max())
    (oracle_logits * gout64).sum().backward()
    PC.fwd_close(ls, oracle_logits.detach().numpy())
    for k, _ in model.named_parameters():
        if sd[k].grad is None:
            assert k not in gs
            continue
        PC.grad_close(gs[k], sd[k].grad.numpy())
        PC.grad_close(gs[k], gt[k].cpu().double().numpy())


def test_gat_train_step_on_a_subgraph_against_twin_graph_and_oracle():
    g = _parent()
    sub, twin = _sub_and_twin(g)
    C = 7
    cfg = dict(n_layers=3, n_heads=3, n_hidden=32, norm="batch", non_interactive_attn=True, use_symmetric_norm=False, linear=True,
               residual=False)
    torch.manual_seed(0)
    model = bnn.GAT(dim_node=24, dim_edge=0, dim_output=C, activation=F.relu, **cfg).to(DEV).train()
    feat = sub.ndata["feat"]
    assert torch.equal(feat, g.ndata["feat"][sub.parent_nid.long()])
    gout64 = torch.randn(feat.shape[0], C, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    gout = gout64.to(DEV, torch.float32)
    sd = _f64(model)
    c0 = fused.CALLS
    on_sub = _step(model, lambda: model(sub, feat), gout)
    assert fused.CALLS > c0                                                         # the fused full-batch layers ran on the subgraph
    on_twin = _step(model, lambda: model(twin, feat), gout)
    s, d = (t.cpu() for t in sub.edges())
    ref = RM.gat_forward(RM.CooGraph(s, d, sub.number_of_nodes()), feat.cpu().double(), sd, n_classes=C, training=True, **cfg)
    _compare(model, on_sub, on_twin, ref, sd, gout64)


def test_gcn_train_step_on_a_subgraph_against_twin_graph_and_oracle():
    g = _parent()
    sub, twin = _sub_and_twin(g)
    C = 7
    torch.manual_seed(0)
    model = bnn.GCN(in_feats=24, n_classes=C, n_hidden=32, n_layers=3, activation=F.relu, norm="batch", norm_adj="symm",
                    dropout=0.0).to(DEV).train()
    feat = sub.ndata["feat"]
    gout64 = torch.randn(feat.shape[0], C, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    gout = gout64.to(DEV, torch.float32)
    sd = _f64(model)
    on_sub = _step(model, lambda: model(sub, feat), gout)
    on_twin = _step(model, lambda: model(twin, feat), gout)
    s, d = (t.cpu() for t in sub.edges())
    ref = RM.gcn_forward(RM.CooGraph(s, d, sub.number_of_nodes()), feat.cpu().double(), sd, n_layers=3, norm="batch", norm_adj="symm",
                         training=True)
    _compare(model, on_sub, on_twin, ref, sd, gout64)


def test_products_gat_train_step_on_a_subgraph_against_twin_graph_and_oracle():
    from bot_amd.nn import edge_gat
    g = _parent()
    sub, twin = _sub_and_twin(g)
    C = 12
    torch.manual_seed(8)
    model = edge_gat.ProductsGAT(node_feats=24, edge_feats=0, n_classes=C, n_layers=3, n_heads=4, n_hidden=20, edge_emb=0,
                                 activation=F.relu, dropout=0.0, input_drop=0.0, attn_drop=0.0, edge_drop=0.0).to(DEV).train()
    feat = sub.ndata["feat"]                                                        # the gathered parent rows, what model(sub) reads
    twin.ndata["feat"] = feat
    gout64 = torch.randn(feat.shape[0], C, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    gout = gout64.to(DEV, torch.float32)
    sd = _f64(model)
    on_sub = _step(model, lambda: model(sub), gout)
    on_twin = _step(model, lambda: model(twin), gout)
    s, d = (t.cpu() for t in sub.edges())
    ref = RM.proteins_gat_forward(RM.CooGraph(s, d, sub.number_of_nodes()), feat.cpu().double(), None, sd, n_layers=3, n_heads=4,
                                  n_hidden=20, training=True, use_node_encoder=False, residual=False)
    _compare(model, on_sub, on_twin, ref, sd, gout64)


@pytest.mark.parametrize("reorder", [None, "degree"])
def test_one_batch_epoch_takes_the_full_batch_step(reorder):
    """ClusterLoader with every part in one batch: train_epoch_subgraphs takes the step train.forward_backward takes on the parent
    with the same mask split (per node) - equal loss (1e-4) and gradients (1e-4 of the largest entry)."""
    n, C, fin = 5000, 6, 16
    rs, rd = synth.powerlaw_edges(n, 50000, 9)
    g = bot_amd.preprocess(bot_amd.Graph(rs, rd, n).to(DEV), reorder=reorder)
    gen = torch.Generator().manual_seed(4)
    feat = torch.randn(n, fin, generator=gen).to(DEV)
    labels = torch.randint(0, C, (n, 1), generator=gen).to(DEV)
    perm = torch.randperm(n, generator=gen).to(DEV)
    tr, va, te = perm[:2700], perm[2700:3600], perm[3600:]
    mask = (torch.rand(2700, generator=gen) < 0.5).to(DEV)
    node_mask = torch.zeros(n, dtype=torch.bool, device=DEV)
    node_mask[tr] = mask
    g.ndata["feat"] = feat
    cfg = dict(n_layers=3, n_heads=2, n_hidden=16, norm="batch", non_interactive_attn=False, use_symmetric_norm=False, linear=True,
               residual=False, dropout=0.0, input_drop=0.0, attn_drop=0.0, edge_drop=0.0)
    torch.manual_seed(1)
    model = bnn.GAT(dim_node=fin + C, dim_edge=0, dim_output=C, activation=F.relu, **cfg).to(DEV)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    kw = dict(use_labels=True, mask_rate=0.5, loss="loge", n_classes=C)
    model.train()
    model.zero_grad(set_to_none=True)
    loss_full, _, _ = T.forward_backward(model, g, feat, labels, tr, va, te, mask=mask, **kw)
    want = {k: p.grad.detach().cpu().double().numpy() for k, p in model.named_parameters()}
    model.load_state_dict(state)                                                    # (BatchNorm's running statistics moved)
    opt = torch.optim.SGD(model.parameters(), lr=0.0)
    loader = ClusterLoader(g, cluster_assignment(g, 4, "random", seed=2), parts_per_batch=4, seed=0)
    c0 = fused.CALLS
    loss_sub, skipped = minibatch.train_epoch_subgraphs(model, loader, opt, labels, tr, val_idx=va, test_idx=te, step_kw=kw,
                                                        node_mask=node_mask)
    assert skipped == 0 and fused.CALLS > c0
    print("loss", float(loss_full.detach()), loss_sub)
    assert abs(float(loss_full) - loss_sub) <= PC.FWD_ATOL
    for k, p in model.named_parameters():
        PC.grad_close(p.grad, want[k])


def test_three_clustered_epochs_of_arxiv_learn():
    from bot_amd import workloads
    torch.manual_seed(0)
    wl = workloads.build_clustered("arxiv", DEV, scale=0.05, seed=0, drop=False)
    assert len(wl.loader) == 30 and wl.step_kw["use_labels"]
    c0 = fused.CALLS
    out = [wl.epoch() for _ in range(3)]
    losses = [v for v, _ in out]
    print("losses", losses, "skipped", [s for _, s in out])
    assert all(math.isfinite(v) for v in losses) and all(s == 0 for _, s in out)
    assert fused.CALLS - c0 >= 3 * 30                                               # every batch ran fused full-batch layers
    assert losses[2] < losses[0], losses
