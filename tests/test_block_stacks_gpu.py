"""The GCN / GAT layers and stacks on sampled blocks on the MI355X (tests/block_cases.py): layers and stacks against the float64
oracle on blocks of the on-device sampler, the fused training nodes and the fused inference layers on blocks (counters), blocks of
the full neighbourhood against the full graph, tuple features, and two seeded sampled epochs of S-arxiv / S-reddit end to end."""
import math

import pytest
import torch

from bot_amd import gemm
from bot_amd.nn import fused
from bot_amd.sampling import MultiLayerFullNeighborSampler, MultiLayerNeighborSampler, NodeDataLoader, sample_block
from tests import block_cases as BC

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _parent():
    return BC.parent_graph(DEV, n=4000, e_raw=30000)


def _block(g):
    seeds = torch.randperm(g.number_of_nodes(), generator=torch.Generator().manual_seed(2))[:700].to(DEV, torch.int32)
    b = sample_block(g, seeds, 5, 77)
    assert b.number_of_src_nodes() > b.number_of_dst_nodes()
    return b


def _blocks(g):
    nids = torch.randperm(g.number_of_nodes(), generator=torch.Generator().manual_seed(3))[:600]
    _, _, blocks = next(iter(NodeDataLoader(g, nids, MultiLayerNeighborSampler([5, 7, 9]), batch_size=600, seed=4)))
    return blocks


@pytest.mark.parametrize("norm", ["both", "right", "none"])
@pytest.mark.parametrize("fin,fout", [(10, 4), (4, 10)])
@pytest.mark.parametrize("train", [True, False])
def test_graphconv_on_a_sampled_block_against_oracle(norm, fin, fout, train):
    BC.check_graphconv_on_block(_block(_parent()), DEV, norm, fin, fout, train)


@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("attn_r", [False, True])
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("train", [True, False])
def test_gatconv_on_a_sampled_block_against_oracle(sym, attn_r, res, train):
    BC.check_gatconv_on_block(_block(_parent()), DEV, sym, attn_r, res, train)


@pytest.mark.parametrize("sym", [False, True])
def test_gatconv_edge_drop_on_a_sampled_block_against_oracle(sym):
    BC.check_gatconv_on_block(_block(_parent()), DEV, sym, True, True, True, keep=True)


def test_tuple_features_on_a_block_and_a_graph():
    g = _parent()
    BC.check_tuple_features(g, _block(g), DEV)


@pytest.mark.parametrize("sym", [False, True])
def test_gat_stack_on_sampled_blocks_against_oracle(monkeypatch, sym):
    monkeypatch.setattr(gemm, "MIN_ROWS", 256)     # these small blocks' projections also run as fp16-halves GEMMs, as at full size
    g = _parent()
    fin = BC.with_labels(g, 8)
    blocks = _blocks(g)
    model = BC.gat_stack(DEV, fin, sym, hidden=20)
    oracle = lambda x, sd: BC.oracle_gat_on_blocks(blocks, x, sd, sym, True, hidden=20)
    c0, a0, l0 = fused.CALLS, fused.AGG_CALLS, fused.L0_CALLS
    fused_out = BC.run_stack_against_oracle(model, blocks, oracle, True)
    assert fused.CALLS - c0 == 3 and fused.AGG_CALLS - a0 == 1
    assert (fused.L0_CALLS > l0) == (not sym)
    model.fuse_layers = False
    BC.close(BC.run_stack_against_oracle(model, blocks, oracle, True), fused_out, 1e-4, "modular = fused")
    model.fuse_layers = True
    i0, li0 = fused.INFER_CALLS, fused.L0_INFER_CALLS
    BC.run_stack_against_oracle(model, blocks, lambda x, sd: BC.oracle_gat_on_blocks(blocks, x, sd, sym, False, hidden=20), False)
    assert fused.INFER_CALLS - i0 == 3
    assert (fused.L0_INFER_CALLS > li0) == (not sym)


@pytest.mark.parametrize("residual", [False, True])
def test_gcn_stack_on_sampled_blocks_against_oracle(residual):
    g = _parent()
    blocks = _blocks(g)
    model = BC.gcn_stack(DEV, 8, residual, use_linear=True)
    for train in (True, False):
        BC.run_stack_against_oracle(model, blocks, lambda x, sd: BC.oracle_gcn_on_blocks(blocks, x, sd, residual, train, True), train)


@pytest.mark.parametrize("kind", ["gat", "gcn"])
@pytest.mark.parametrize("train", [True, False])
def test_full_neighbourhood_blocks_equal_the_full_graph(kind, train):
    g = _parent()
    n = g.number_of_nodes()
    fin = BC.with_labels(g, 8) if kind == "gat" else 8
    _, out_nodes, blocks = next(iter(NodeDataLoader(g, torch.arange(n), MultiLayerFullNeighborSampler(3), batch_size=n, seed=1)))
    assert torch.equal(out_nodes.cpu(), torch.arange(n)) and all(b.number_of_src_nodes() == n for b in blocks)
    model = BC.gat_stack(DEV, fin, True) if kind == "gat" else BC.gcn_stack(DEV, fin, True)
    model.train(train)
    feat = g.ndata["feat"]
    with torch.set_grad_enabled(train):
        full = model(g, feat)
        on_blocks = model(blocks)
    BC.close(on_blocks, full, 1e-5, "logits")
    if train:
        full.sum().backward()
        gf = {k: p.grad.clone() for k, p in model.named_parameters()}
        model.zero_grad(set_to_none=True)
        model(blocks).sum().backward()
        for k, p in model.named_parameters():
            scale = float(gf[k].abs().max())
            if scale < 1e-6:      # a bias in front of a training-mode BatchNorm: zero in exact arithmetic
                assert float(p.grad.abs().max()) < 1e-5, k
            else:
                BC.close(p.grad, gf[k], 1e-5, k)


@pytest.mark.parametrize("name,scale", [("arxiv", 0.05), ("reddit", 0.004)])
def test_two_sampled_epochs_are_finite_and_reproducible(name, scale):
    from bot_amd import workloads
    params, calls = [], []
    for _ in range(2):
        torch.manual_seed(0)
        wl = workloads.build_sampled(name, DEV, scale=scale, seed=0)
        assert len(wl.loader) >= 2
        c0 = fused.CALLS
        losses = [wl.epoch() for _ in range(2)]
        assert all(math.isfinite(v) for v in losses), losses
        calls.append(fused.CALLS - c0)
        params.append([p.detach().clone() for p in wl.model.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*params))
    assert calls[0] == (6 * len(wl.loader) if name == "arxiv" else 0)      # the GAT's three layers take the fused nodes on every batch
