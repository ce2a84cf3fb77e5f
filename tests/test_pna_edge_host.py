"""PNA with edge features without a GPU: the tensor form of `ops.pna_aggregate_edge` on CPU tensors over the emulated backend
(tests/_oracle_backend.py, tests/sage_cases.py) against the float64 restatement (tests/pna_edge_cases.py) under the suite's criteria;
owners, empty rows, the tower layout, K above the kernel's limit, the gradient of `ef`; `nn.EdgePNAConv` / `nn.EdgePNA` with their
state_dict keys, every argument error, `workloads.build_pna_edge`, the new entry points' argument checks through the C ABI, and the
reason for the SPLIT pivot: in float32 a single pivot a_0 + c_0 fails the variance bound once `a` is shifted, the split pivot does
not.  tests/test_pna_edge_gpu.py holds the kernels to the same restatements.

The first two tests call nothing under test: one checks the restatement against the edge-less one and against itself, the other states
the design's reason by simulating both pivots in numpy float32 - it does not hold the kernel to that order (the GPU suite's bounds at
a + 1000 do).  They pass with or without the feature; every other test here needs it."""
import ctypes
import inspect
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import bot_amd
from bot_amd import nn as bnn
from bot_amd import ops, workloads
from bot_amd.errors import DGLError
from tests import _oracle_backend
from tests import block_cases as BC
from tests import pna_cases as PC
from tests import pna_edge_cases as PE
from tests import sage_cases as SG
from tests.parity_cases import fwd_close, grad_close

ALL6 = ("mean", "sum", "max", "min", "std", "var")


@pytest.fixture
def backend(monkeypatch):
    _oracle_backend.install(monkeypatch)
    SG.install(monkeypatch)


def _operands(g, F_, K, seed):
    gen = torch.Generator().manual_seed(seed)
    a = torch.randn(g.number_of_src_nodes(), F_, generator=gen)
    b = torch.randn(g.number_of_dst_nodes(), F_, generator=gen)
    ef = torch.randn(g.number_of_edges(), K, generator=gen)
    w = torch.randn(F_, K, generator=gen)
    return a, b, ef, w


# ------------------------------------------------------------------------------------------------ the restatement itself
def test_restatement_reduces_to_the_edge_less_one_and_its_two_forms_agree():
    g = SG.small_graph(65, 90, 1)
    indptr, indices = SG.csc_of(g)
    a, b, ef, w = (t.numpy() for t in _operands(g, 8, 3, 0))
    ef_pos = ef[PE.position_rows(g)]
    vals0, own0, info0 = PE.aggregate(indptr, indices, a, ef_pos, np.zeros_like(w), b)
    _, ref, info = PC.aggregate(indptr, indices, a, b, ALL6)
    for k in ALL6:
        np.testing.assert_allclose(vals0[k], ref[k], rtol=0, atol=1e-12)
    amax, amin = PC.owners(indptr, indices, a)
    assert np.array_equal(own0[0], amax) and np.array_equal(own0[1], amin)
    np.testing.assert_allclose(info0["D"], info["dmax"], atol=0) and np.testing.assert_allclose(info0["asum"], info["asum"], atol=1e-12)
    for Ft in (8, 4):
        out, (amax, amin) = PE.forward(indptr, indices, a, ef_pos, w, b, ALL6, PC.SCALERS3, 1.3, Ft)
        t64 = lambda x: torch.from_numpy(x).double()
        t = PE.pna_edge_torch(indptr, indices, t64(a), t64(b), t64(ef_pos), t64(w), ALL6, PC.SCALERS3, 1.3, Ft)
        np.testing.assert_allclose(t.numpy(), out, rtol=0, atol=1e-11)              # the numpy loops and the torch ops agree
        t = PE.pna_edge_torch(indptr, indices, t64(a), t64(b), t64(ef_pos), t64(w), ALL6, PC.SCALERS3, 1.3, Ft, amax, amin)
        np.testing.assert_allclose(t.numpy(), out, rtol=0, atol=1e-11)              # ... evaluated at the owners as well
    SG.check_arg(indptr, amax)
    SG.check_arg(indptr, amin)
    # the edge term moves owners: they are those of a + c, not of a
    assert not np.array_equal(amax, PC.owners(indptr, indices, a)[0])


def test_a_single_pivot_fails_the_variance_bound_once_shifted_and_the_split_pivot_does_not():
    """Why the kernel keeps p_a and p_c apart.  In float32 the deviation from the single pivot fl(a_0 + c_0) is fl(fl(a_k + c_k) - P):
    both messages are rounded at the ulp of 1000 first.  The split deviation fl(fl(a_k - p_a) + fl(c_k - p_c)) is made of numbers of
    the size of the spread, shifted or not."""
    g = SG.small_graph(65, 90, 3)
    indptr, indices = SG.csc_of(g)
    rng = np.random.default_rng(1)
    base = rng.standard_normal((90, 6))
    ef = rng.standard_normal((g.number_of_edges(), 3)).astype(np.float32)
    w = rng.standard_normal((6, 3)).astype(np.float32)
    ef_pos = ef[PE.position_rows(g)]
    c32 = np.zeros((len(ef_pos), 6), dtype=np.float32)
    for k in range(len(ef_pos)):                                       # the contract's chain: a rounded product, then fused multiply-adds
        s = (ef_pos[k, 0] * w[:, 0]).astype(np.float32)
        for j in (1, 2):
            s = (s.astype(np.float64) + ef_pos[k, j].astype(np.float64) * w[:, j].astype(np.float64)).astype(np.float32)
        c32[k] = s
    for shift in (0.0, 1000.0):
        a = (base + shift).astype(np.float32)
        vals, _, info = PE.aggregate(indptr, indices, a, ef_pos, w, None)
        bound = PE.bounds(info, 3)["var"]
        one, split = np.zeros_like(vals["var"]), np.zeros_like(vals["var"])
        for r in range(65):
            lo, hi = indptr[r], indptr[r + 1]
            if hi == lo:
                continue
            n = np.float32(hi - lo)
            rows, cr = a[indices[lo:hi]], c32[lo:hi]
            P = rows[0] + cr[0]
            s1 = s2 = d1 = d2 = np.zeros(6, dtype=np.float32)
            for x, c in zip(rows, cr):                                 # position-order float32 sums
                e = (x + c) - P
                d = (x - rows[0]) + (c - cr[0])
                s1, s2, d1, d2 = s1 + e, s2 + e * e, d1 + d, d2 + d * d
            one[r] = np.maximum(s2 / n - (s1 / n) * (s1 / n), 0)
            split[r] = np.maximum(d2 / n - (d1 / n) * (d1 / n), 0)
        assert bool((np.abs(split - vals["var"]) <= bound).all())
        if shift:
            assert not bool((np.abs(one - vals["var"]) <= bound).all())


# ------------------------------------------------------------------------------------------------ the op on CPU tensors
@pytest.mark.parametrize("towers", (1, 2, 4))
@pytest.mark.parametrize("with_b", (True, False))
def test_tensor_form_against_the_restatement(backend, towers, with_b):
    for g, K in ((SG.small_graph(65, 90, 7), 3), (SG.small_graph(40, 40, 8), 17)):          # (17: above the kernel's limit)
        indptr, indices = SG.csc_of(g)
        n_dst, F_ = g.number_of_dst_nodes(), 8
        a, b, ef, w = (t.requires_grad_() for t in _operands(g, F_, K, 1))
        b = b if with_b else None
        out, saved, sarg = ops.pna_aggregate_edge(g, a, b, ef, w, ALL6, PC.SCALERS3, 1.4, tower_width=F_ // towers, return_saved=True)
        assert out.shape == (n_dst, 3 * 6 * F_) and sarg.dtype == torch.int32 and not saved.requires_grad
        rows = torch.from_numpy(PE.position_rows(g))
        ef_pos = ef.detach()[rows].numpy()
        want, (amax, amin) = PE.forward(indptr, indices, a.detach().numpy(), ef_pos, w.detach().numpy(),
                                        None if b is None else b.detach().numpy(), ALL6, PC.SCALERS3, 1.4, F_ // towers)
        fwd_close(out, want)
        assert np.array_equal(sarg[:, :F_].numpy(), amax) and np.array_equal(sarg[:, F_:].numpy(), amin)
        vals, _, _ = PE.aggregate(indptr, indices, a.detach().numpy(), ef_pos, w.detach().numpy(), None)
        fwd_close(saved[:, :F_], vals["mean"])                                                # the messages' mean, without b
        deg = np.diff(indptr)
        assert bool((out.detach().numpy()[deg == 0] == 0).all()) and (deg == 0).any()       # an empty row: zeros, no b
        assert bool((sarg.numpy()[deg == 0] == -1).all()) and bool((saved.numpy()[deg == 0] == 0).all())
        dout = torch.randn(out.shape, generator=torch.Generator().manual_seed(2))
        out.backward(dout)
        a64, w64, e64 = (t.detach().double().requires_grad_() for t in (a, w, ef))
        b64 = None if b is None else b.detach().double().requires_grad_()
        PE.pna_edge_torch(indptr, indices, a64, b64, e64[rows], w64, ALL6, PC.SCALERS3, 1.4, F_ // towers, amax, amin).backward(dout.double())
        grad_close(a.grad, a64.grad.numpy())
        grad_close(w.grad, w64.grad.numpy())
        grad_close(ef.grad, e64.grad.numpy())
        if with_b:
            grad_close(b.grad, b64.grad.numpy())
    assert "pna_aggregate_edge" in ops.__all__ and ops.pna_edge_default_impl in ops.PNA_IMPLS


def test_tensor_form_rows_of_one_neighbour_and_of_constant_messages_have_zero_variance(backend):
    g = SG.small_graph(65, 90, 9)
    indptr, indices = SG.csc_of(g)
    deg = np.diff(indptr)
    assert (deg == 1).any()
    a, b, ef, w = _operands(g, 4, 3, 4)
    out, saved, _ = ops.pna_aggregate_edge(g, a, b, ef, w, ("var", "std"), ("identity",), return_saved=True)
    one = torch.from_numpy(deg == 1)
    assert bool((out[one][:, :4] == 0).all()) and bool((saved[one][:, 4:] == 0).all())


def test_argument_errors(backend):
    g = SG.small_graph(20, 30, 8)
    E = g.number_of_edges()
    a, b, ef, w = _operands(g, 8, 4, 0)
    assert ops.pna_aggregate_edge(g, a, b, ef, w).shape == (20, 3 * 4 * 8)
    assert ops.pna_aggregate_edge(g, a, None, ef, w, aggregators=("var",), scalers=("identity",)).shape == (20, 8)
    with pytest.raises(NotImplementedError, match="moment"):
        ops.pna_aggregate_edge(g, a, b, ef, w, aggregators=("mean", "moment3"))
    with pytest.raises(DGLError):
        ops.pna_aggregate_edge(g, a, b, ef, w, aggregators=("median",))
    with pytest.raises(DGLError):
        ops.pna_aggregate_edge(g, a, b, ef, w, scalers=("linear",))
    with pytest.raises(ValueError, match="tower_width"):
        ops.pna_aggregate_edge(g, a, b, ef, w, tower_width=3)
    with pytest.raises(ValueError, match="source nodes"):
        ops.pna_aggregate_edge(g, a[:-1], b, ef, w)
    with pytest.raises(ValueError, match=r"\[n_src, F\]"):
        ops.pna_aggregate_edge(g, a.reshape(30, 2, 4), b, ef, w)
    with pytest.raises(ValueError, match="n_dst"):
        ops.pna_aggregate_edge(g, a, b[:-1], ef, w)
    with pytest.raises(ValueError, match=r"ef must be \[\d+, K >= 1\] \(one row per edge, edge-id order\)"):
        ops.pna_aggregate_edge(g, a, b, ef[:-1], w)
    with pytest.raises(ValueError, match="ef must be"):
        ops.pna_aggregate_edge(g, a, b, ef.reshape(-1), w)
    with pytest.raises(ValueError, match="ef must be"):
        ops.pna_aggregate_edge(g, a, b, None, w)
    with pytest.raises(ValueError, match=r"weight must be \[8, 4\]"):
        ops.pna_aggregate_edge(g, a, b, ef, w.t())
    with pytest.raises(ValueError, match="ef must be torch.float32"):
        ops.pna_aggregate_edge(g, a, b, ef.double(), w)
    with pytest.raises(ValueError, match="weight must be torch.float32"):
        ops.pna_aggregate_edge(g, a, b, ef, w.double())
    with pytest.raises(ValueError, match="impl"):
        ops.pna_aggregate_edge(g, a, b, ef, w, impl="triton")
    part = BC.parent_graph("cpu", n=200, e_raw=1500, seed=7)
    x = torch.randn(200, 8)
    conv = bnn.EdgePNAConv(8, 8, ["mean"], ["identity"], 1.0, edge_feat_size=4)
    pe = torch.randn(part.number_of_edges(), 4)
    assert conv(part, x, pe).shape == (200, 8)
    with pytest.raises(ValueError, match="edge_feat must be"):
        conv(part, x, None)
    with pytest.raises(ValueError, match="edge_feat must be"):
        conv(part, x, pe[:, :3])
    with pytest.raises(ValueError, match="edge_feat must be"):
        conv(part, x, pe[:-1])
    with pytest.raises(ValueError, match="source nodes"):
        conv(part, x[:100], pe)
    with pytest.raises(ValueError, match="destination"):
        conv(part, (x, x[:19]), pe)
    for bad in (0, -1):
        with pytest.raises(ValueError, match="edge_feat_size"):
            bnn.EdgePNAConv(8, 8, ["mean"], ["identity"], 1.0, edge_feat_size=bad)
    with pytest.raises(DGLError, match="num_towers"):
        bnn.EdgePNAConv(8, 8, ["mean"], ["identity"], 1.0, num_towers=3, edge_feat_size=2)
    with pytest.raises(NotImplementedError, match="moment"):
        bnn.EdgePNAConv(8, 8, ["moment3"], ["identity"], 1.0, edge_feat_size=2)
    part.halo = object()                                             # a partition's block carries a halo plan
    with pytest.raises(ValueError, match="partition"):
        conv(part, x, pe)
    with pytest.raises(ValueError, match="partition"):
        ops.pna_aggregate_edge(part, x, None, pe, torch.randn(8, 4))
    # PNAConv keeps refusing, and now says where the feature lives
    with pytest.raises(NotImplementedError, match="EdgePNAConv"):
        bnn.PNAConv(8, 8, ["mean"], ["identity"], 1.0, edge_feat_size=4)
    with pytest.raises(NotImplementedError, match="EdgePNAConv"):
        bnn.PNAConv(8, 8, ["mean"], ["identity"], 1.0)(g, a, edge_feat=ef)


# ------------------------------------------------------------------------------------------------ EdgePNAConv, EdgePNA, the recipe
def test_state_dict_keys_and_shapes():
    conv = bnn.EdgePNAConv(16, 24, ["mean", "max", "sum"], ["identity", "amplification"], 2.5, num_towers=2, edge_feat_size=5)
    assert {k: tuple(v.shape) for k, v in conv.state_dict().items()} == PE.conv_keys(16, 24, 2, 5, 6)
    assert conv.towers[0].M.weight.shape == (8, 2 * 8 + 5) and conv.edge_feat_size == 5 and not conv.residual
    assert bnn.EdgePNAConv(16, 16, ["mean"], ["identity"], 1.0, edge_feat_size=1).residual
    model = bnn.EdgePNA(8, 5, 12, 3, edge_dim=4, num_towers=2)
    keys = set(model.state_dict())
    assert {"encoder.weight", "decoder.bias", "convs.2.towers.1.M.weight", "convs.0.mixing_layer.0.bias"} <= keys
    assert model.convs[1].towers[1].M.weight.shape == (6, 16) and model.edge_dim == 4 and len(model.convs) == 3
    assert {"EdgePNAConv", "EdgePNA"} <= set(bnn.__all__)
    # PNAConv's parameters are what they were
    assert bnn.PNAConv(16, 24, ["mean"], ["identity"], 1.0, num_towers=2).towers[0].M.weight.shape == (8, 16)


@pytest.mark.parametrize("towers", (1, 2))
def test_edge_pnaconv_against_fp64_restatement(backend, monkeypatch, towers):
    g = BC.parent_graph("cpu")
    PE.check_conv(g, "cpu", monkeypatch, 8, 8, towers, 3)
    seeds = torch.randperm(g.number_of_nodes(), generator=torch.Generator().manual_seed(3))[:150]
    b = BC.host_blocks(g, seeds, (5,), 0)[0]
    assert b.number_of_src_nodes() > b.number_of_dst_nodes()
    PE.check_conv(b, "cpu", monkeypatch, 8, 12, towers, 3, seed=1)
    PE.check_conv(SG.small_graph(65, 65, 10), "cpu", monkeypatch, 8, 8, towers, 3, residual=False, seed=2)      # isolated destinations


def test_edge_pnaconv_takes_a_feature_pair(backend):
    b = SG.small_graph(30, 50, 11)
    torch.manual_seed(0)
    conv = bnn.EdgePNAConv(8, 8, PC.AGGS4, PC.SCALERS3, 1.5, dropout=0.5, num_towers=2, edge_feat_size=3).eval()
    hs, hd, ef = torch.randn(50, 8), torch.randn(30, 8), torch.randn(b.number_of_edges(), 3)
    out = conv(b, (hs, hd), ef)
    p = {k: v.detach().double() for k, v in conv.named_parameters()}
    ef_pos = ef.double()[torch.from_numpy(PE.position_rows(b))]
    ref = PE.edge_pna_conv(conv, *SG.csc_of(b), hs.double(), hd.double(), ef_pos, p)
    fwd_close(out, ref.numpy())
    conv.train()
    assert conv(b, (hs, hd), ef).shape == (30, 8) and int(conv.towers[0].batchnorm.num_batches_tracked) == 1


def test_edge_pna_stack_against_fp64_restatement(backend, monkeypatch):
    g = BC.parent_graph("cpu")
    ef = torch.rand(g.number_of_edges(), 4, generator=torch.Generator().manual_seed(2))
    torch.manual_seed(3)
    model = bnn.EdgePNA(8, 5, 12, 3, edge_dim=4, delta=bnn.pna_delta(g), num_towers=2, dropout=0.5)
    PE.check_stack(model, g, g.ndata["feat"], ef, "cpu", monkeypatch)
    monkeypatch.undo()
    _oracle_backend.install(monkeypatch)
    SG.install(monkeypatch)
    # the three ways a Graph hands its edge features over give the same output
    g.edata["feat"], g.edata["other"] = ef, ef
    with torch.no_grad():
        x, y, z = model(g, g.ndata["feat"], ef), model(g, g.ndata["feat"]), model(g, g.ndata["feat"], "other")
    assert torch.equal(x, y) and torch.equal(x, z)
    seeds = torch.randperm(g.number_of_nodes(), generator=torch.Generator().manual_seed(3))[:150]
    blocks = BC.host_blocks(g, seeds, (4, 5, 6), 0)
    per_block = [b.edata["feat"] for b in blocks]
    assert all(e.shape == (b.number_of_edges(), 4) for e, b in zip(per_block, blocks))
    model2 = bnn.EdgePNA(8, 5, 12, 3, edge_dim=4, delta=1.5)
    PE.check_stack(model2, blocks, blocks[0].srcdata["feat"], per_block, "cpu", monkeypatch)
    with torch.no_grad():
        assert torch.equal(model2(blocks), model2(blocks, None, per_block))
    with pytest.raises(ValueError, match="one per block"):
        model2(blocks, None, per_block[:2])
    del g.edata["feat"]
    with pytest.raises(ValueError, match="edata"):
        model(g, g.ndata["feat"])


def test_build_pna_edge_full_batch_step(backend):
    wl = workloads.build_pna_edge("proteins", "cpu", scale=0.002, drop=False)       # (the CPU emulation has no dropout stream)
    assert isinstance(wl.model, bnn.EdgePNA) and len(wl.model.convs) == 3 and wl.model.convs[0].out_size == 256
    assert wl.model.edge_dim == 8 and wl.dataset.efeat.shape[1] == 8 and wl.dataset.n_classes == 112
    assert wl.dominant == ("spmm_pna_edge", (256, 256, 8, 3, 4)) and "edge_dim 8" in wl.describe
    assert wl.model.convs[0].aggregators == PC.AGGS4 and wl.model.convs[0].scalers == PC.SCALERS3
    assert abs(wl.model.convs[0].delta - bnn.pna_delta(wl.graph)) < 1e-6
    loss, pred = wl.step()
    assert bool(torch.isfinite(loss)) and pred.shape == (wl.n_nodes, 112) and bool(torch.isfinite(pred).all())
    params = dict(wl.model.named_parameters())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params.values())
    assert all(float(params[f"convs.{i}.towers.0.M.weight"].grad[:, 512:].abs().max()) > 0 for i in range(3))     # the edge columns learn


def test_build_pna_edge_shapes_and_refusals():
    sig = inspect.signature(workloads.build_pna_edge)
    assert [p for p in sig.parameters][:2] == ["name", "device"]
    assert {k: v.default for k, v in sig.parameters.items() if v.kind is v.KEYWORD_ONLY} == dict(
        sampled=False, scale=1.0, seed=0, drop=True, num_towers=1)
    for name in ("cora", "arxiv", "reddit", "products", "nothing"):
        with pytest.raises(ValueError, match="build_pna_edge"):
            workloads.build_pna_edge(name, "cpu")
    with pytest.raises(ValueError):
        workloads.build_pna("proteins", "cpu")              # build_pna is what it was


# ------------------------------------------------------------------------------------------------ the C ABI's checks, no GPU
def test_argument_validation_without_gpu():
    from bot_amd import _C
    lib = _C._lib
    codes = lambda *c: (ctypes.c_int32 * len(c))(*c)
    four = codes(0, 2, 3, 4)
    buf = torch.zeros(1024)
    p = buf.data_ptr()
    assert p % 16 == 0

    def fwd(**k):
        aggs = k.get("aggs", four)
        return lib.bot_spmm_pna_edge_f32(k.get("indptr"), None, k.get("n", 4), k.get("nnz", 0), k.get("items"), 4, None, None, 0, 0, k.get("a"),
                                         k.get("lda", 4), None, 0, k.get("F", 4), k.get("Ft", 4), k.get("ef"), k.get("K", 8), k.get("eperm"),
                                         k.get("wt", p + 2048), None if aggs is None else ctypes.addressof(aggs), k.get("A", 4), None,
                                         k.get("S", 1), k.get("out"), k.get("ldo", 16), None, 0, None, 0, None, None)

    def bwd(**k):
        aggs = k.get("aggs", four)
        return lib.bot_spmm_pna_edge_bwd_f32(None, None, k.get("n", 4), k.get("nnz", 0), k.get("items"), 4, None, None, 0, None, k.get("a"),
                                             k.get("lda", 4), k.get("ef"), k.get("K", 8), k.get("eperm"), k.get("wt", p + 2048), k.get("rec"),
                                             k.get("ldr", 28), None if aggs is None else ctypes.addressof(aggs), 4, k.get("F", 4),
                                             k.get("dx", p + 256), k.get("ldx", 4), None, k.get("dweight"), k.get("dw_ws"),
                                             k.get("dw_rows", 0), None)
    for f in (fwd, bwd):
        assert f(F=0) == -2 and b"F=0" in lib.bot_last_error()
        assert f(n=-1) == -2
        assert f() == -1 and b"NULL" in lib.bot_last_error()                   # NULL operands
        assert f(aggs=None) == -1 and b"aggs" in lib.bot_last_error()
        assert f(aggs=codes(0, 2, 9, 4)) == -2 and b"unknown aggregator code 9" in lib.bot_last_error()
        for K in (0, 17, -1):
            assert f(K=K) == -2 and f"K={K} (1 .. 16)".encode() in lib.bot_last_error()
        assert f(wt=None) == -1 and b"ef/wt" in lib.bot_last_error()
        assert f(nnz=3) == -1 and b"ef/wt" in lib.bot_last_error()             # edges without ef
        assert f(wt=p + 2050) == -3 and f(ef=p + 2, nnz=3) == -3 and f(eperm=p + 2) == -3
        assert f(n=0) == 0                                                     # an empty problem is a no-op
    assert fwd(Ft=3) == -2 and b"tower width" in lib.bot_last_error() and fwd(Ft=0) == -2
    assert fwd(S=0) == -2 and fwd(A=9) == -2 and fwd(A=0) == -2
    ok = dict(indptr=p, items=p, a=p + 64, out=p + 256)
    assert fwd(**ok, lda=3) == -2 and b"stride" in lib.bot_last_error()        # strides below F
    assert fwd(**ok, ldo=15) == -2 and b"stride" in lib.bot_last_error()
    assert fwd(indptr=p, items=p, a=p + 64, out=p + 64) == -2 and b"alias" in lib.bot_last_error()
    assert fwd(indptr=p, items=p, a=p + 64, out=p + 2048) == -2 and b"alias" in lib.bot_last_error()      # out == wt
    assert fwd(**ok, S=2) == -1 and b"scale" in lib.bot_last_error()
    okb = dict(items=p, a=p, rec=p + 64)
    assert bwd(**okb, ldx=3) == -2 and b"stride" in lib.bot_last_error()
    assert bwd(**okb, ldr=27) == -2 and bwd(**okb, lda=3) == -2                # the record of mean, max, min, std has 7 sections
    assert bwd(items=p, rec=p + 64) == -1 and b"std / var need a" in lib.bot_last_error()
    assert bwd(**okb, dw_rows=-1) == -2
    assert bwd(**okb, dweight=p + 512) == -1 and b"dw_workspace" in lib.bot_last_error()
    assert bwd(**okb, dweight=p + 512, dw_ws=p + 1024, dw_rows=0) == -2 and b"workgroup partials" in lib.bot_last_error()
    assert bwd(**okb, dx=None) == 0                                            # neither gradient asked for: nothing to do
    assert _C.PNA_EDGE_MAX_K == 16


def test_abi_is_still_19_and_the_new_symbols_are_in_header_and_binding():
    from bot_amd import _C
    header = (Path(bot_amd.__file__).resolve().parent.parent / "include" / "bot_gnn.h").read_text()
    declared = set(re.findall(r"\b(bot_\w+)\s*\(", header))
    new = {"bot_spmm_pna_edge_f32", "bot_spmm_pna_edge_bwd_f32"}
    assert new <= declared and new <= set(_C.EXPORTED) and new <= set(_C._SIGS)
    assert all(hasattr(_C._lib, name) for name in new)
    assert _C._lib.bot_abi_version() == 19 == _C.ABI_VERSION
    assert all(callable(getattr(_C, name)) for name in ("spmm_pna_edge", "spmm_pna_edge_bwd"))
