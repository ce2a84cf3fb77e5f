"""Edge-weighted neighbour sampling on the MI355X (csrc/sampling_weighted.hip, bot_amd.sampling with `prob`): the sampler bit for
bit against the numpy restatement of tests/test_weighted_sampling_host.py (a hub of 10^5 in-edges, zero, subnormal and huge
weights, shuffled seeds), the rejection of invalid weights, the cache of prepared weights, the block structure, stack parity on
weighted blocks against the oracle, and two seeded weighted epochs end to end."""
import math

import numpy as np
import pytest
import torch

import bot_amd
from bot_amd import _C
from bot_amd.sampling import MultiLayerNeighborSampler, NodeDataLoader, sample_block
from tests.test_sampling_gpu import _close, _graph_with_hub, _oracle_stack, _parent, _stack
from tests.test_weighted_sampling_host import quantise_row, weighted_reference

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _hub_weights(g, gen):
    """Uniform weights with 20 % zeros, plus rows (by destination) of all-zero, subnormal and near-1e38 weights."""
    E = g.number_of_edges()
    w = torch.rand(E, generator=gen)
    w[torch.rand(E, generator=gen) < 0.2] = 0
    d = g.edges()[1].cpu()
    w[(d >= 100) & (d < 160)] = 0                                                # rows whose weights are all zero
    sub = (d >= 200) & (d < 260)
    w[sub] = torch.rand(int(sub.sum()), generator=gen) * 1e-39                   # subnormal (below 1.18e-38)
    big = (d >= 300) & (d < 360)
    w[big] = torch.rand(int(big.sum()), generator=gen) * 3e38
    return w


def test_weighted_sampler_bit_exact_against_the_numpy_restatement():
    s, d, n = _graph_with_hub()
    g = bot_amd.Graph(s, d, n).to(DEV)
    csc = g.csc
    indptr = csc.indptr.cpu().numpy().astype(np.int64)
    eid = csc.eid.cpu().numpy().astype(np.int64)
    deg = np.diff(indptr)
    gen = torch.Generator().manual_seed(21)
    w = _hub_weights(g, gen)
    wn = w.numpy()
    assert deg.max() >= 100000 and (deg == 0).sum() >= 200
    assert np.any((wn > 0) & (wn < 1.17e-38)) and wn.max() > 1e38
    prepared = _C.sample_weights_prepare(csc, w.to(DEV))
    n_pos = np.array([int(np.count_nonzero(quantise_row(wn[eid[indptr[v]:indptr[v + 1]]]))) for v in range(n)])
    assert np.array_equal(prepared.n_pos.cpu().numpy(), n_pos)
    q_all = np.concatenate([quantise_row(wn[eid[indptr[v]:indptr[v + 1]]]) for v in range(n)])
    row_of = np.repeat(np.arange(n), deg)
    starts = np.r_[0, np.cumsum(deg)[:-1]]
    cs = np.cumsum(q_all, dtype=np.uint64)
    ref_prefix = cs - np.where(starts[row_of] > 0, cs[np.maximum(starts[row_of] - 1, 0)], np.uint64(0))
    assert np.array_equal(prepared.prefix.cpu().numpy().view(np.uint64), ref_prefix)
    assert torch.equal(_C.sample_weights_prepare(csc, w.to(DEV).reshape(-1, 1)).prefix, prepared.prefix)   # [E, 1] as [E]

    extra = torch.tensor([7, n - 1, n - 2, 120, 130, 210, 220, 310, 320])        # hub, no in-edges, all-zero, subnormal, huge rows
    seeds = torch.randperm(n, generator=gen)[:2500]
    seeds = torch.cat([extra, seeds[~torch.isin(seeds, extra)]])
    seeds = seeds[torch.randperm(seeds.numel(), generator=gen)]
    assert n_pos[7] > 1024 and n_pos[120] == 0 and deg[120] > 0
    seeds_d = seeds.to(DEV, torch.int32)
    for k in (1, 8, 100, 1024, -1):
        seed = 0x0F1E2D3C4B5A6978 + k
        off, pos = _C.sample_neighbors_weighted(csc, prepared, seeds_d, k, seed)
        ro, rp = weighted_reference(indptr, eid, wn, seeds.numpy(), k, seed)
        assert np.array_equal(off.cpu().numpy(), ro), k
        assert np.array_equal(pos.cpu().numpy().astype(np.int64), rp), k
        assert np.all(wn[eid[rp]] > 0), k                                             # zero weights never taken
        off2, pos2 = _C.sample_neighbors_weighted(csc, prepared, seeds_d, k, seed)
        assert torch.equal(off, off2) and torch.equal(pos, pos2)
        # purity: the rows do not depend on where a seed sits in the list
        perm = torch.randperm(seeds.numel(), generator=gen)
        off3, pos3 = _C.sample_neighbors_weighted(csc, prepared, seeds_d[perm.to(DEV)].contiguous(), k, seed)
        off, pos, off3, pos3 = off.cpu(), pos.cpu(), off3.cpu(), pos3.cpu()
        for j in range(0, seeds.numel(), 97):
            i = int(perm[j])
            assert torch.equal(pos3[off3[j]:off3[j + 1]], pos[off[i]:off[i + 1]]), (k, j)
        if k > 0:
            _, pos4 = _C.sample_neighbors_weighted(csc, prepared, seeds_d, k, seed + 1)
            assert not torch.equal(pos.to(DEV), pos4), k


def test_prepare_rejects_invalid_weights():
    g = _parent(n=500, e_raw=3000)
    E = g.number_of_edges()
    for bad in (-1.0, float("nan"), float("inf"), float("-inf")):
        w = torch.rand(E, device=DEV)
        w[E // 2] = bad
        with pytest.raises(ValueError):
            _C.sample_weights_prepare(g.csc, w)
    with pytest.raises(ValueError):
        _C.sample_weights_prepare(g.csc, torch.rand(E + 1, device=DEV))
    ok = _C.sample_weights_prepare(g.csc, torch.rand(E, device=DEV))                 # the flag is reset per preparation
    assert int(ok.n_pos.sum()) <= E
    g.edata["w"] = torch.rand(E, device=DEV)
    g.edata["w"][3] = -2.0
    with pytest.raises(ValueError):
        sample_block(g, torch.arange(10, dtype=torch.int32, device=DEV), 4, 1, prob="w")


def test_prepared_weights_are_cached_and_see_in_place_changes():
    g = _parent()
    n, E = g.number_of_nodes(), g.number_of_edges()
    csc = g.csc
    indptr, eid = csc.indptr.cpu().numpy().astype(np.int64), csc.eid.cpu().numpy().astype(np.int64)
    g.edata["w"] = torch.rand(E, generator=torch.Generator().manual_seed(4)).to(DEV)
    seeds = torch.randperm(n, generator=torch.Generator().manual_seed(5))[:800]
    sd = seeds.to(DEV, torch.int32)

    def check(b, k, s):
        ro, rp = weighted_reference(indptr, eid, g.edata["w"].cpu().numpy(), seeds.numpy(), k, s)
        assert np.array_equal(b.parent_eid.cpu().numpy().astype(np.int64), eid[rp])

    b1 = sample_block(g, sd, 3, 17, prob="w")
    check(b1, 3, 17)
    cached = g._bot_prob_cache[1]
    sample_block(g, sd, 3, 18, prob="w")
    assert g._bot_prob_cache[1] is cached                                             # unchanged weights: no new preparation
    g.edata["w"].mul_((torch.rand(E, generator=torch.Generator().manual_seed(6)) < 0.5).float().to(DEV))   # in place
    b2 = sample_block(g, sd, 3, 17, prob="w")
    assert g._bot_prob_cache[1] is not cached
    check(b2, 3, 17)
    assert not torch.equal(b1.parent_eid, b2.parent_eid)
    wt = g.edata["w"].clone()                                                         # a tensor works as well as a key
    b3 = sample_block(g, sd, 3, 17, prob=wt)
    assert torch.equal(b3.parent_eid, b2.parent_eid)


def test_weighted_blocks_of_a_three_layer_loader():
    g = _parent()
    n, E = g.number_of_nodes(), g.number_of_edges()
    ps, pd = (t.cpu() for t in g.edges())
    gen = torch.Generator().manual_seed(7)
    w = 0.1 + torch.rand(E, generator=gen)
    w[torch.rand(E, generator=gen) < 0.3] = 0
    g.edata["w"] = w.to(DEV)
    pos_deg = torch.bincount(pd[w > 0], minlength=n)
    nids = torch.randperm(n, generator=torch.Generator().manual_seed(1))[:1500]
    fan = [4, 6, 8]
    loader = NodeDataLoader(g, nids, MultiLayerNeighborSampler(fan, prob="w"), batch_size=400, shuffle=True, seed=9)
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
            assert torch.all(sid[nd:][1:] > sid[nd:][:-1])
            if i + 1 < len(blocks):
                assert torch.equal(blocks[i + 1].src_nid.cpu(), b.dst_nid.cpu())
            bs, bd = (t.cpu() for t in b.edges())
            pe = b.parent_eid.long().cpu()
            assert torch.equal(ps[pe], sid[bs]) and torch.equal(pd[pe], sid[bd])
            assert int(torch.unique(pe).numel()) == pe.numel()
            assert bool((w[pe] > 0).all())
            assert torch.equal(b.srcdata["feat"], g.ndata["feat"][b.src_nid.long()])
            assert torch.equal(b.edata["feat"], g.edata["feat"][b.parent_eid.long()])
            assert torch.equal(b.edata["w"], g.edata["w"][b.parent_eid.long()])
            deg = torch.bincount(bd, minlength=nd)
            npos = pos_deg[b.dst_nid.long().cpu()]
            assert torch.equal(deg, torch.minimum(npos, torch.full_like(npos, fan[i])))
    seen = torch.cat(seen)
    assert seen.numel() == nids.numel() and torch.equal(torch.sort(seen).values, torch.sort(nids).values)
    assert bool((g._bot_block_map.cpu() == -1).all())


@pytest.mark.parametrize("kind", ["proteins", "products"])
def test_stack_on_weighted_blocks_against_oracle(kind):
    g = _parent(efeat=kind == "proteins")
    E = g.number_of_edges()
    g.edata["w"] = torch.rand(E, generator=torch.Generator().manual_seed(12)).to(DEV) ** 3
    nids = torch.randperm(g.number_of_nodes(), generator=torch.Generator().manual_seed(3))[:600]
    _, out_nodes, blocks = next(iter(NodeDataLoader(g, nids, MultiLayerNeighborSampler([5, 7, 9], prob="w"), batch_size=600, seed=4)))
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


@pytest.mark.parametrize("name,scale", [("products", 0.002), ("proteins", 0.02)])
def test_two_weighted_sampled_epochs_are_finite_and_reproducible(name, scale):
    from bot_amd import workloads
    params = []
    for _ in range(2):
        torch.manual_seed(0)
        wl = workloads.build_sampled(name, DEV, scale=scale, seed=0, prob=True)
        assert "edge-weighted" in wl.describe and wl.loader.sampler.prob == workloads.SAMPLED_WEIGHT
        w = wl.graph.edata[workloads.SAMPLED_WEIGHT]
        assert w.shape == (wl.graph.number_of_edges(),) and bool((w > 0).all())
        assert len(wl.loader) >= 2
        losses = [wl.epoch() for _ in range(2)]
        assert all(math.isfinite(v) for v in losses), losses
        params.append([p.detach().clone() for p in wl.model.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*params))
