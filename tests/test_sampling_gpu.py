"""Neighbour sampling, blocks and mini-batch training on the MI355X (bot_amd.sampling, csrc/sampling.hip, the block branch of
bot_amd/nn/edge_gat.py, bot_amd.minibatch): the sampler bit for bit against the numpy restatement of tests/test_sampling_host.py,
the block structure, layer and stack parity on blocks against the oracle, blocks of the full neighbourhood against the full graph,
and two seeded epochs end to end."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bot_amd
from bot_amd import _C
from bot_amd.sampling import MultiLayerFullNeighborSampler, MultiLayerNeighborSampler, NodeDataLoader, sample_block
from oracle import ref_models as RM
from tests.test_sampling_host import sample_reference

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _graph_with_hub(n=6000, e_raw=40000, hub_deg=120000, seed=3):
    """Power-law graph + one hub of in-degree >= 10^5 (node 7) + a range of nodes with no in-edges at all (the last 200)."""
    gen = torch.Generator().manual_seed(seed)
    m = n - 200
    src = (m * torch.rand(e_raw, generator=gen, dtype=torch.float64) ** 2.0).long().clamp_(max=m - 1)
    dst = (m * torch.rand(e_raw, generator=gen, dtype=torch.float64) ** 2.0).long().clamp_(max=m - 1)
    hs = torch.randint(0, n, (hub_deg,), generator=gen)
    src, dst = torch.cat([src, hs]), torch.cat([dst, torch.full((hub_deg,), 7)])
    perm = torch.randperm(e_raw + hub_deg, generator=gen)
    return src[perm], dst[perm], n


def _close(a, b, tol, what=""):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    scale = max(float(b.abs().max()), 1e-30) if b.numel() else 1.0
    err = float((a - b).abs().max()) / scale if b.numel() else 0.0
    assert a.shape == b.shape and err <= tol, (what, tuple(a.shape), tuple(b.shape), err)


def test_sampler_bit_exact_against_the_numpy_restatement():
    s, d, n = _graph_with_hub()
    g = bot_amd.Graph(s, d, n).to(DEV)
    csc = g.csc
    indptr = csc.indptr.cpu().numpy().astype(np.int64)
    deg = np.diff(indptr)
    assert deg.max() >= 100000 and (deg == 0).sum() >= 200
    gen = torch.Generator().manual_seed(11)
    extra = torch.tensor([7, n - 1, n - 2])                                     # the hub and two rows without in-edges
    seeds = torch.randperm(n, generator=gen)[:2500]
    seeds = torch.cat([extra, seeds[~torch.isin(seeds, extra)]])
    seeds = seeds[torch.randperm(seeds.numel(), generator=gen)]                  # unique, in random order
    assert bool((seeds == 7).any()) and bool((torch.from_numpy(deg)[seeds] == 0).any())
    seeds_d = seeds.to(DEV, torch.int32)
    for k in (1, 8, 32, 100, -1):
        seed = 0x0123456789ABCDEF + k
        off, pos = _C.sample_neighbors(csc, seeds_d, k, seed)
        ro, rp = sample_reference(indptr, seeds.numpy(), k, seed)
        assert np.array_equal(off.cpu().numpy(), ro), k
        assert np.array_equal(pos.cpu().numpy().astype(np.int64), rp), k
        off2, pos2 = _C.sample_neighbors(csc, seeds_d, k, seed)
        assert torch.equal(off, off2) and torch.equal(pos, pos2)
        if k > 0:
            _, pos3 = _C.sample_neighbors(csc, seeds_d, k, seed + 1)
            assert not torch.equal(pos, pos3), k


def _parent(n=4000, e_raw=30000, seed=5, efeat=True):
    from oracle import ref_ops as R
    from bot_amd import synth
    rs, rd = synth.powerlaw_edges(n, e_raw, seed)
    s, d = R.preprocess_edges(rs, rd, n)
    g = bot_amd.Graph(s, d, n).to(DEV)
    gen = torch.Generator().manual_seed(seed + 1)
    g.ndata["feat"] = torch.randn(n, 8, generator=gen).to(DEV)
    if efeat:
        g.edata["feat"] = torch.rand(s.numel(), 8, generator=gen).to(DEV)
    return g


def test_blocks_of_a_three_layer_loader():
    g = _parent()
    n = g.number_of_nodes()
    ps, pd = (t.cpu() for t in g.edges())
    nids = torch.randperm(n, generator=torch.Generator().manual_seed(1))[:1500]
    loader = NodeDataLoader(g, nids, MultiLayerNeighborSampler([4, 6, 8]), batch_size=400, shuffle=True, seed=9)
    seen = []
    for input_nodes, output_nodes, blocks in loader:
        assert len(blocks) == 3 and torch.equal(input_nodes, blocks[0].src_nid.long())
        assert torch.equal(blocks[-1].dst_nid.long(), output_nodes)
        seen.append(output_nodes.cpu())
        for i, b in enumerate(blocks):
            assert b.is_block and b.halo is None
            nd, ns = b.number_of_dst_nodes(), b.number_of_src_nodes()
            sid = b.src_nid.long().cpu()
            assert torch.equal(sid[:nd], b.dst_nid.long().cpu())
            assert int(torch.unique(sid).numel()) == ns
            assert torch.all(sid[nd:][1:] > sid[nd:][:-1])                    # new sources in ascending parent id
            if i + 1 < len(blocks):
                assert torch.equal(blocks[i + 1].src_nid.cpu(), b.dst_nid.cpu())
            bs, bd = (t.cpu() for t in b.edges())
            pe = b.parent_eid.long().cpu()
            assert torch.equal(ps[pe], sid[bs]) and torch.equal(pd[pe], sid[bd])
            assert int(torch.unique(pe).numel()) == pe.numel()
            assert torch.equal(b.srcdata["feat"], g.ndata["feat"][b.src_nid.long()])
            assert torch.equal(b.dstdata["feat"], g.ndata["feat"][b.dst_nid.long()])
            assert torch.equal(b.edata["feat"], g.edata["feat"][b.parent_eid.long()])
            deg = torch.bincount(bd, minlength=nd)
            pdeg = torch.bincount(pd, minlength=n)[b.dst_nid.long().cpu()]
            assert torch.equal(deg, torch.minimum(pdeg, torch.full_like(pdeg, [4, 6, 8][i])))
    seen = torch.cat(seen)
    assert seen.numel() == nids.numel() and torch.equal(torch.sort(seen).values, torch.sort(nids).values)
    assert bool((_C_map(g) == -1).all())


def _C_map(g):
    return g._bot_block_map.cpu()


def _coo(b):
    s, d = (t.cpu() for t in b.edges())
    return RM.CooGraph(s, d, b.number_of_src_nodes())


def _conv(kind):
    from bot_amd.nn import edge_gat
    torch.manual_seed(3)
    if kind == "proteins":
        conv = edge_gat.GATConv(48, 16, 8, n_heads=6, allow_zero_in_degree=True)
        enc = torch.nn.Linear(8, 16)
    else:
        conv = edge_gat.GATConv(48, 0, 30, n_heads=4, allow_zero_in_degree=True)
        enc = None
    return conv.to(DEV), (enc.to(DEV) if enc is not None else None)


@pytest.mark.parametrize("kind", ["proteins", "products"])
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_gatconv_on_a_sampled_block_against_oracle(kind, mode):
    g = _parent(efeat=kind == "proteins")
    seeds = torch.randperm(g.number_of_nodes(), generator=torch.Generator().manual_seed(2))[:700].to(DEV, torch.int32)
    b = sample_block(g, seeds, 5, 77)
    nd, ns = b.number_of_dst_nodes(), b.number_of_src_nodes()
    assert ns > nd
    conv, enc = _conv(kind)
    conv.train(mode == "train")
    x = torch.randn(ns, 48, generator=torch.Generator().manual_seed(4)).to(DEV)
    ef = b.edata["feat"] if kind == "proteins" else None
    gout = torch.randn(nd, conv._n_heads, conv._out_feats, generator=torch.Generator().manual_seed(6)).to(DEV)
    sd = {k: v.detach().cpu().double().requires_grad_() for k, v in conv.state_dict().items()}
    esd = {k: v.detach().cpu().double().requires_grad_() for k, v in enc.state_dict().items()} if enc is not None else {}
    xr = x.cpu().double().requires_grad_()
    emb = F.relu(F.linear(ef.cpu().double(), esd["weight"], esd["bias"])) if enc is not None else None
    ref = RM.proteins_gatconv_forward(_coo(b), xr, sd, "", n_heads=conv._n_heads, out_feats=conv._out_feats, feat_edge=emb)[:nd]
    (ref * gout.cpu().double()).sum().backward()
    if mode == "eval":
        with torch.no_grad():
            out = conv(b, x, ef, edge_encoder=enc)
        _close(out, ref, 2e-5, "eval out")
        return
    xg = x.clone().requires_grad_()
    out = conv(b, xg, ef, edge_encoder=enc)
    assert out.shape == (nd, conv._n_heads, conv._out_feats)
    _close(out, ref, 2e-5, "out")
    (out * gout).sum().backward()
    _close(xg.grad, xr.grad, 2e-4, "dx")
    for k, p in conv.named_parameters():
        _close(p.grad, sd[k].grad, 2e-4, k)
    if enc is not None:
        for k, p in enc.named_parameters():
            _close(p.grad, esd[k].grad, 2e-4, "enc." + k)


def _stack(kind, n_layers=3):
    from bot_amd.nn import edge_gat
    torch.manual_seed(8)
    if kind == "proteins":
        m = edge_gat.ProteinsGAT(node_feats=8, edge_feats=8, n_classes=12, n_layers=n_layers, n_heads=6, n_hidden=16, edge_emb=16,
                                 activation=F.relu, dropout=0.0, input_drop=0.0, attn_drop=0.0, edge_drop=0.0, allow_zero_in_degree=True)
    else:
        m = edge_gat.ProductsGAT(node_feats=8, edge_feats=0, n_classes=12, n_layers=n_layers, n_heads=4, n_hidden=20, edge_emb=0,
                                 activation=F.relu, dropout=0.0, input_drop=0.0, attn_drop=0.0, edge_drop=0.0)
    return m.to(DEV)


def _oracle_stack(kind, blocks, sd, n_layers=3):
    """The reference's block branch (ogbn-proteins/models.py:235-264) composed per layer from the oracle's layer: the block as an
    n_src-node graph (rows >= n_dst have no in-edges) sliced to n_dst, BatchNorm over those rows, residual h_last[:n_dst]."""
    heads, hid = (6, 16) if kind == "proteins" else (4, 20)
    h = blocks[0].srcdata["feat"].cpu().double()
    if kind == "proteins":
        h = F.relu(F.linear(h, sd["node_encoder.weight"], sd["node_encoder.bias"]))
    h_last = None
    for i, b in enumerate(blocks):
        nd = b.number_of_dst_nodes()
        emb = None
        if kind == "proteins":
            emb = F.relu(F.linear(b.edata["feat"].cpu().double(), sd[f"edge_encoder.{i}.weight"], sd[f"edge_encoder.{i}.bias"]))
        h = RM.proteins_gatconv_forward(_coo(b), h, sd, f"convs.{i}.", n_heads=heads, out_feats=hid, feat_edge=emb)[:nd].flatten(1)
        if kind == "proteins" and h_last is not None:
            h = h + h_last[:nd]
        h_last = h
        h = F.relu(F.batch_norm(h, None, None, sd[f"norms.{i}.weight"], sd[f"norms.{i}.bias"], training=True))
    return F.linear(h, sd["pred_linear.weight"], sd["pred_linear.bias"])


@pytest.mark.parametrize("kind", ["proteins", "products"])
def test_stack_on_blocks_against_oracle(kind):
    g = _parent(efeat=kind == "proteins")
    nids = torch.randperm(g.number_of_nodes(), generator=torch.Generator().manual_seed(3))[:600]
    _, out_nodes, blocks = next(iter(NodeDataLoader(g, nids, MultiLayerNeighborSampler([5, 7, 9]), batch_size=600, seed=4)))
    model = _stack(kind)
    model.train()
    sd = {k: v.detach().cpu().double().requires_grad_() for k, v in model.state_dict().items() if v.is_floating_point()}
    pred = model(blocks)
    ref = _oracle_stack(kind, blocks, sd)
    _close(pred, ref, 1e-4, "logits")
    gout = torch.randn(ref.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    (pred * gout.to(DEV, torch.float32)).sum().backward()
    (ref * gout).sum().backward()
    for k, p in model.named_parameters():
        if kind == "products" and k.startswith("node_encoder"):
            assert p.grad is None
            continue
        if k.endswith("dst_fc.bias"):        # zero in exact arithmetic (in front of a training-mode BatchNorm): held to the weight's scale
            scale = float(sd[k.replace("bias", "weight")].grad.abs().max())
            assert float((p.grad.double().cpu() - sd[k].grad).abs().max()) <= 2e-4 * scale, k
            continue
        _close(p.grad, sd[k].grad, 2e-4, k)


@pytest.mark.parametrize("kind", ["proteins", "products"])
@pytest.mark.parametrize("mode", ["train", "eval"])
def test_full_neighbourhood_blocks_equal_the_full_graph(kind, mode):
    g = _parent(efeat=kind == "proteins")
    n = g.number_of_nodes()
    loader = NodeDataLoader(g, torch.arange(n), MultiLayerFullNeighborSampler(3), batch_size=n, seed=1)
    _, out_nodes, blocks = next(iter(loader))
    assert torch.equal(out_nodes.cpu(), torch.arange(n)) and all(b.number_of_src_nodes() == n for b in blocks)
    model = _stack(kind)
    model.train(mode == "train")
    with torch.set_grad_enabled(mode == "train"):
        full = model(g)
        on_blocks = model(blocks)
    _close(on_blocks, full, 1e-5, "logits")
    if mode == "train":
        full.sum().backward()
        gf = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
        model.zero_grad(set_to_none=True)
        model(blocks).sum().backward()
        for k, p in model.named_parameters():
            if k.endswith("dst_fc.bias"):    # zero in exact arithmetic (in front of a training-mode BatchNorm): held to the weight's scale
                scale = float(gf[k.replace("bias", "weight")].abs().max())
                assert float((p.grad - gf[k]).abs().max()) <= 1e-4 * scale, k
            elif k in gf:
                _close(p.grad, gf[k], 1e-4, k)


@pytest.mark.parametrize("name,scale", [("products", 0.002), ("proteins", 0.02)])
def test_two_sampled_epochs_are_finite_and_reproducible(name, scale):
    from bot_amd import workloads
    params = []
    for _ in range(2):
        torch.manual_seed(0)
        wl = workloads.build_sampled(name, DEV, scale=scale, seed=0)
        assert len(wl.loader) >= 2
        losses = [wl.epoch() for _ in range(2)]
        assert all(math.isfinite(v) for v in losses), losses
        params.append([p.detach().clone() for p in wl.model.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*params))
