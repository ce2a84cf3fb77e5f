"""The GCN / GAT layers and stacks on sampled blocks without a GPU: the emulated backend (tests/_oracle_backend.py) under the host
logic, blocks built by tests/block_cases.host_blocks, the fused nodes forced on (fused.FORCE; with gemm.FORCE the fp16-halves forms
too).  tests/test_block_stacks_gpu.py runs the same checks on the MI355X with the on-device sampler."""
import pytest
import torch

from bot_amd.nn import fused
from tests import _oracle_backend
from tests import block_cases as BC


@pytest.fixture()
def cpu_backend(monkeypatch):
    _oracle_backend.install(monkeypatch)
    monkeypatch.setattr(fused, "FORCE", True)


def _blocks(g, n_seeds=150, fanouts=(4, 5, 6), seed=0):
    seeds = torch.randperm(g.number_of_nodes(), generator=torch.Generator().manual_seed(seed + 3))[:n_seeds]
    return BC.host_blocks(g, seeds, fanouts, seed)


@pytest.mark.parametrize("norm", ["both", "right", "none"])
@pytest.mark.parametrize("fin,fout", [(10, 4), (4, 10)])
@pytest.mark.parametrize("train", [True, False])
def test_graphconv_on_a_block_against_oracle(cpu_backend, norm, fin, fout, train):
    g = BC.parent_graph("cpu")
    b = _blocks(g, fanouts=(5,))[0]
    assert b.number_of_src_nodes() > b.number_of_dst_nodes()
    BC.check_graphconv_on_block(b, "cpu", norm, fin, fout, train)


@pytest.mark.parametrize("sym", [False, True])
@pytest.mark.parametrize("attn_r", [False, True])
@pytest.mark.parametrize("res", [False, True])
@pytest.mark.parametrize("train", [True, False])
def test_gatconv_on_a_block_against_oracle(cpu_backend, sym, attn_r, res, train):
    g = BC.parent_graph("cpu")
    b = _blocks(g, fanouts=(5,))[0]
    BC.check_gatconv_on_block(b, "cpu", sym, attn_r, res, train)


@pytest.mark.parametrize("sym", [False, True])
def test_gatconv_edge_drop_on_a_block(cpu_backend, sym):
    g = BC.parent_graph("cpu")
    b = _blocks(g, fanouts=(5,))[0]
    BC.check_gatconv_on_block(b, "cpu", sym, True, True, True, keep=True)


def test_tuple_features(cpu_backend):
    g = BC.parent_graph("cpu")
    BC.check_tuple_features(g, _blocks(g, fanouts=(5,))[0], "cpu")


@pytest.mark.parametrize("halves", [False, True])
@pytest.mark.parametrize("sym", [False, True])
def test_gat_stack_on_blocks_against_oracle(cpu_backend, monkeypatch, sym, halves):
    from bot_amd import gemm
    if halves:
        monkeypatch.setattr(gemm, "FORCE", True)
    g = BC.parent_graph("cpu")
    fin = BC.with_labels(g, 8)
    blocks = _blocks(g)
    model = BC.gat_stack("cpu", fin, sym)
    oracle = lambda x, sd: BC.oracle_gat_on_blocks(blocks, x, sd, sym, True)
    c0, a0, l0 = fused.CALLS, fused.AGG_CALLS, fused.L0_CALLS
    fused_out = BC.run_stack_against_oracle(model, blocks, oracle, True)
    assert fused.CALLS - c0 == 3 and fused.AGG_CALLS - a0 == 1
    assert (fused.L0_CALLS > l0) == (not sym)      # the grouped-halves form of the aggregate-first node (forced on the emulated backend)
    model.fuse_layers = False
    BC.close(BC.run_stack_against_oracle(model, blocks, oracle, True), fused_out, 1e-4, "modular = fused")
    model.fuse_layers = True
    i0, li0 = fused.INFER_CALLS, fused.L0_INFER_CALLS
    eval_oracle = lambda x, sd: BC.oracle_gat_on_blocks(blocks, x, sd, sym, False)
    BC.run_stack_against_oracle(model, blocks, eval_oracle, False)
    assert fused.INFER_CALLS - i0 == 3
    assert (fused.L0_INFER_CALLS > li0) == (not sym)


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("use_linear", [False, True])
def test_gcn_stack_on_blocks_against_oracle(cpu_backend, residual, use_linear):
    g = BC.parent_graph("cpu")
    blocks = _blocks(g)
    model = BC.gcn_stack("cpu", 8, residual, use_linear)
    for train in (True, False):
        BC.run_stack_against_oracle(model, blocks, lambda x, sd: BC.oracle_gcn_on_blocks(blocks, x, sd, residual, train, use_linear), train)


def test_stacks_check_the_block_count(cpu_backend):
    g = BC.parent_graph("cpu")
    blocks = _blocks(g, fanouts=(4, 5))
    with pytest.raises(ValueError):
        BC.gcn_stack("cpu", 8, False)(blocks)
    with pytest.raises(ValueError):
        BC.gat_stack("cpu", 8, False)(blocks)


@pytest.mark.parametrize("kind", ["gat", "gcn"])
@pytest.mark.parametrize("train", [True, False])
def test_full_neighbourhood_blocks_equal_the_full_graph(cpu_backend, kind, train):
    g = BC.parent_graph("cpu")
    n = g.number_of_nodes()
    fin = BC.with_labels(g, 8) if kind == "gat" else 8
    blocks = BC.host_blocks(g, torch.arange(n), (-1, -1, -1))
    assert all(b.number_of_src_nodes() == n for b in blocks)
    model = BC.gat_stack("cpu", fin, True) if kind == "gat" else BC.gcn_stack("cpu", fin, True)
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
