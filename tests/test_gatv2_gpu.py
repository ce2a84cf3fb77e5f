"""GATv2 on the MI355X: the three sweeps of csrc/gatv2.hip against the float64 restatement (tests/gatv2_cases.py) - entry for entry on
integer-valued inputs, whose sums are exact in float32 whatever their order, and under bounds derived from the lengths on seeded normal
inputs - the kernel form against the tensor form, `nn.GATv2Conv` and `nn.GATv2` against their float64 restatements under the suite's
own criteria (tests/parity_cases.py), and the steps of `workloads.build_gatv2`.

Largest error seen as a fraction of its derived bound (run with -s to print them): DESIGN §8 "GATv2"."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bot_amd import _C, ops, workloads
from bot_amd import nn as bnn
from bot_amd.errors import DGLError
from bot_amd.sampling import MultiLayerNeighborSampler, NodeDataLoader, sample_block
from tests import block_cases as BC
from tests import gatv2_cases as GC
from tests import sage_cases as SG

pytestmark = pytest.mark.gpu
DEV = "cuda"
# (1, 1) the smallest; (1, 3) odd width, 4-byte lanes; (3, 5) heads that end inside a group at odd lanes; (4, 65) heads straddling
# 64-lane chunks; (3, 250) the workload's width (one tile of six chunks; with an odd row stride it walks tiles with heads that span
# them, as (1, 1000) does)
PAIRS = ((1, 1), (1, 3), (3, 5), (2, 64), (8, 32), (4, 65), (3, 250), (1, 1000))
WORST = {}


@functools.lru_cache(maxsize=None)
def _graphs():
    """(name, graph on the device): 1 / 63 / 64 / 65 square rows with isolated rows and parallel edges, chunk = 4 variants (long rows: the
    workspace and the combine at small sizes), and a block with n_src > n_dst."""
    out = [(f"square{n}", SG.small_graph(n, n, n).to(DEV)) for n in (1, 63, 64, 65)]
    out.append(("long65", SG.small_graph(65, 65, 70, chunk=4).to(DEV)))
    out.append(("block", SG.small_graph(63, 200, 71).to(DEV)))
    out.append(("longblock", SG.small_graph(64, 130, 72, chunk=4).to(DEV)))
    for i in (4, 6):
        assert out[i][1].csc.n_long > 0 and out[i][1].csr.n_long > 0
    assert out[0][1].csc.n_long == 0
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _hub():
    from tests.test_subgraph_gpu import _hub_graph
    g = _hub_graph()
    assert int(np.diff(g.csc.indptr.cpu().numpy()).max()) > 2048 and g.csc.n_long > 0 and g.csr.n_long > 0
    return g


def _slab(t, pad, fill=7.0):
    """A device view of the [n, ..] tensor `t` whose rows sit in a buffer `pad` floats wider (row stride width + pad)."""
    n, w = t.shape[0], t[0].numel() if t.shape[0] else int(np.prod(t.shape[1:]))
    buf = torch.full((n, w + pad), fill, dtype=t.dtype, device=DEV)
    buf[:, :w].copy_(t.reshape(n, w).to(DEV))
    return buf[:, :w].view(t.shape), buf


def _same_bytes(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _eq(got, want):
    return np.array_equal(got.detach().cpu().double().numpy(), want.numpy())


def _check_exact(g, H, D, slope, pad, seed, **ranges):
    """The three entry points on integer-valued inputs, entry for entry; strided operands and outputs with `pad`."""
    E, n_src, n_dst = g.number_of_edges(), g.number_of_src_nodes(), g.number_of_dst_nodes()
    fs, fd, attn, de = GC.integer_inputs(n_src, n_dst, E, H, D, seed, **ranges)
    want_e, want_dfs, want_dfd, want_dattn = GC.exact_reference(g, fs, fd, attn, slope, de)
    (fsd, _), (fdd, _), atd, (ded, _) = _slab(fs, pad), _slab(fd, pad), attn.to(DEV), _slab(de, pad)
    csc, csr = g.csc, g.csr
    e_out, e_buf = _slab(torch.full((E, H), 9.0), pad, 9.0)
    e = _C.gatv2_logits(csc, fsd, fdd, atd, slope, out=e_out if pad else None)
    assert "gatv2_logits_kernel" in _C._lib.bot_last_kernel().decode()
    assert _eq(e, want_e), (H, D, slope, pad)
    assert _same_bytes(_C.gatv2_logits(csc, fsd, fdd, atd, slope), e)
    by_eid = _C.gatv2_logits(csc, fsd, fdd, atd, slope, operm=csc.eid)
    assert torch.equal(by_eid[csc.eid.long()], e.contiguous())                     # edge-id order is the CSC order permuted by csc.eid
    dfd_out, dfd_buf = _slab(torch.full((n_dst, H, D), 9.0), pad, 9.0)
    dfd, dattn = _C.gatv2_logits_bwd_dst(csc, fsd, fdd, atd, slope, ded, out=dfd_out if pad else None)
    assert "gatv2_logits_bwd_kernel<1" in _C._lib.bot_last_kernel().decode()
    assert _eq(dfd, want_dfd) and _eq(dattn, want_dattn), (H, D, slope, pad)
    dfd2, dattn2 = _C.gatv2_logits_bwd_dst(csc, fsd, fdd, atd, slope, ded)
    assert _same_bytes(dfd2, dfd) and _same_bytes(dattn2, dattn)
    only_fd, none = _C.gatv2_logits_bwd_dst(csc, fsd, fdd, atd, slope, ded, want_dattn=False)
    none2, only_at = _C.gatv2_logits_bwd_dst(csc, fsd, fdd, atd, slope, ded, want_dfd=False)
    assert none is None and none2 is None and _same_bytes(only_fd, dfd) and _same_bytes(only_at, dattn)
    dfs_out, dfs_buf = _slab(torch.full((n_src, H, D), 9.0), pad, 9.0)
    dfs = _C.gatv2_logits_bwd_src(csr, g.csr2csc, fsd, fdd, atd, slope, ded, out=dfs_out if pad else None)
    assert "gatv2_logits_bwd_kernel<0" in _C._lib.bot_last_kernel().decode()
    assert _eq(dfs, want_dfs), (H, D, slope, pad)
    assert _same_bytes(_C.gatv2_logits_bwd_src(csr, g.csr2csc, fsd, fdd, atd, slope, ded), dfs)
    # de in edge-id order through the permutations gives the same bytes
    de_eid = torch.empty_like(ded.contiguous())
    de_eid[csc.eid.long()] = ded
    assert _same_bytes(_C.gatv2_logits_bwd_dst(csc, fsd, fdd, atd, slope, de_eid, dperm=csc.eid)[0], dfd)
    assert _same_bytes(_C.gatv2_logits_bwd_src(csr, csr.eid, fsd, fdd, atd, slope, de_eid), dfs)
    if pad:                                                                         # nothing is written beyond a strided row
        w = H * D
        assert bool((e_buf[:, H:] == 9.0).all()) and bool((dfd_buf[:, w:] == 9.0).all()) and bool((dfs_buf[:, w:] == 9.0).all())


# ------------------------------------------------------------------------------------------------ 1. exact
@pytest.mark.parametrize("H,D", PAIRS)
def test_logits_and_gradients_are_exact_on_integers(H, D):
    for i, (name, g) in enumerate(_graphs()):
        for slope, pad in ((0.5, 0), (0.25, 0), (0.5, 3), (0.25, 4)):
            _check_exact(g, H, D, slope, pad, seed=17 * i + H + D + pad)


def test_logits_and_gradients_are_exact_on_the_hub_graph():
    """Rows above 2 048 in-edges at the default chunk; the ranges are shrunk so that every sum's absolute terms stay below 2^22."""
    g = _hub()
    for (H, D), slope in (((3, 5), 0.5), ((2, 8), 0.25)):
        _check_exact(g, H, D, slope, 0, seed=H, lim=1, de_lim=1, de_keep=0.125)


def test_autograd_orders_and_needed_gradients(monkeypatch):
    name, g = _graphs()[6]
    E, n_src, n_dst = g.number_of_edges(), g.number_of_src_nodes(), g.number_of_dst_nodes()
    fs, fd, attn, de = GC.integer_inputs(n_src, n_dst, E, 3, 5, 1)
    want = GC.exact_reference(g, fs, fd, attn, 0.5, de)
    eid = g.csc.eid.long()
    for order in ("csc", "eid"):
        leaves = [t.clone().to(DEV).requires_grad_() for t in (fs, fd, attn.view(1, 3, 5))]
        e = ops.gatv2_logits(g, *leaves, negative_slope=0.5, order=order)
        assert e.shape == (E, 3, 1)
        up = de.to(DEV)
        if order == "eid":
            up = torch.empty_like(up)
            up[eid] = de.to(DEV)
            assert _eq(e.view(E, 3)[eid], want[0])
        else:
            assert _eq(e.view(E, 3), want[0])
        e.backward(up.view(E, 3, 1))
        assert _eq(leaves[0].grad, want[1]) and _eq(leaves[1].grad, want[2]) and _eq(leaves[2].grad.view(3, 5), want[3])
    # each gradient is computed only when asked for; the CSR is touched only for dfs
    calls = []
    real_dst, real_src = _C.gatv2_logits_bwd_dst, _C.gatv2_logits_bwd_src
    monkeypatch.setattr(_C, "gatv2_logits_bwd_dst", lambda *a, **k: (calls.append(("dst", k["want_dfd"], k["want_dattn"])), real_dst(*a, **k))[1])
    monkeypatch.setattr(_C, "gatv2_logits_bwd_src", lambda *a, **k: (calls.append(("src",)), real_src(*a, **k))[1])
    g2 = SG.small_graph(20, 30, 8).to(DEV)
    x = [torch.randn(30, 2, 4, device=DEV), torch.randn(20, 2, 4, device=DEV), torch.randn(2, 4, device=DEV)]
    for need, seen in (((False, True, False), [("dst", True, False)]), ((False, False, True), [("dst", False, True)]),
                       ((False, True, True), [("dst", True, True)])):
        calls.clear()
        leaves = [t.clone().requires_grad_(r) for t, r in zip(x, need)]
        ops.gatv2_logits(g2, *leaves).sum().backward()
        assert calls == seen and g2._csr is None
    calls.clear()
    leaves = [t.clone().requires_grad_(r) for t, r in zip(x, (True, False, False))]
    ops.gatv2_logits(g2, *leaves).sum().backward()
    assert calls == [("src",)] and g2._csr is not None


# ------------------------------------------------------------------------------------------------ 2. rounded, and the two forms
@pytest.mark.parametrize("H,D", PAIRS)
def test_kernel_and_tensor_forms_against_fp64_under_derived_bounds(H, D):
    for i in (3, 4, 5, 6):
        name, g = _graphs()[i]
        got_k, bnd = GC.check_op(g, DEV, H, D, seed=i + H * D, impl="kernel", worst=WORST)
        got_t, _ = GC.check_op(g, DEV, H, D, seed=i + H * D, impl="tensor")
        for a, b, lim in zip(got_k, got_t, bnd):                      # the two forms agree within the sum of both forms' bounds
            assert bool(((a - b).abs() <= 2 * lim).all())
    GC.check_op(_graphs()[6][1], DEV, H, D, seed=5, order="eid", impl="kernel", worst=WORST)
    print("largest error / bound so far:", {k: round(v, 4) for k, v in WORST.items()})


def test_hub_graph_against_fp64_under_derived_bounds(monkeypatch):
    GC.check_op(_hub(), DEV, 3, 5, seed=2, impl="kernel", worst=WORST)
    monkeypatch.setenv("BOT_GATV2", "tensor")                        # read at call time
    calls = []
    real = _C.gatv2_logits
    monkeypatch.setattr(_C, "gatv2_logits", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    GC.check_op(_graphs()[5][1], DEV, 3, 5, seed=2)
    assert calls == []
    monkeypatch.delenv("BOT_GATV2")
    GC.check_op(_graphs()[5][1], DEV, 3, 5, seed=2)
    assert calls == [1] and ops.gatv2_default_impl == "kernel"
    print("largest error / bound so far:", {k: round(v, 4) for k, v in WORST.items()})


# ------------------------------------------------------------------------------------------------ 3. the layer
@functools.lru_cache(maxsize=None)
def _parent():
    return BC.parent_graph(DEV, n=4000, e_raw=30000)


@functools.lru_cache(maxsize=None)
def _block():
    g = _parent()
    seeds = torch.randperm(g.number_of_nodes(), generator=torch.Generator().manual_seed(2))[:700].to(DEV, torch.int32)
    b = sample_block(g, seeds, 5, 77)
    assert b.number_of_src_nodes() > b.number_of_dst_nodes()
    return b


@functools.lru_cache(maxsize=None)
def _subgraph():
    g = _parent()
    nodes = torch.randperm(g.number_of_nodes(), generator=torch.Generator().manual_seed(4))[:1500].sort().values
    return g.subgraph(nodes.to(DEV))


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("bias", [False, True])
def test_gatv2conv_against_fp64_restatement(residual, bias):
    kw = dict(residual=residual, bias=bias)
    GC.check_conv(_parent(), DEV, 8, 3, 5, **kw)
    GC.check_conv(_parent(), DEV, 8, 2, 4, seed=1, share_weights=True, **kw)
    GC.check_conv(_subgraph(), DEV, 8, 3, 5, seed=2, allow_zero_in_degree=True, **kw)
    b = _block()
    GC.check_conv(b, DEV, (8, 6), 2, 8, seed=3, pair=True, allow_zero_in_degree=True, **kw)
    GC.check_conv(b, DEV, 8, 2, 4, seed=4, share_weights=True, allow_zero_in_degree=True, **kw)
    GC.check_conv(b, DEV, 8, 1, 8, seed=5, allow_zero_in_degree=True, **kw)        # in == H * D: the identity residual


def test_attention_dropout_zeroes_weight_and_gradient_together():
    g = _parent()
    conv = GC.make_conv(8, 2, 4, 0, attn_drop=0.5).to(DEV).train()
    seen = []

    def keep(module, inputs, output):
        inputs[0].retain_grad()
        seen.extend((inputs[0], output))
    conv.attn_drop.register_forward_hook(keep)
    torch.manual_seed(1)
    x = torch.randn(g.number_of_nodes(), 8, device=DEV, requires_grad=True)
    out = conv(g, x)
    out.backward(torch.randn(out.shape, device=DEV))
    a, dropped = seen
    assert 0.3 < float((dropped == 0).float().mean()) < 0.7
    assert torch.equal(a.grad == 0, dropped == 0)                     # a weight the mask zeroed gets no gradient, every other one does
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(x.grad).all())
    assert all(bool(torch.isfinite(p.grad).all()) for p in conv.parameters())


# ------------------------------------------------------------------------------------------------ 4. the stack and the recipes
def test_gatv2_stack_against_fp64_restatement():
    g = _parent()
    torch.manual_seed(3)
    model = bnn.GATv2(8, 5, 6, 3, 2, F.relu, norm="batch", dropout=0.5, attn_drop=0.1)
    GC.check_stack(model, g, g.ndata["feat"].cpu(), DEV)
    nids = torch.randperm(g.number_of_nodes(), generator=torch.Generator().manual_seed(3))[:600]
    _, _, blocks = next(iter(NodeDataLoader(g, nids, MultiLayerNeighborSampler([5, 7, 9]), batch_size=600, seed=4)))
    model2 = bnn.GATv2(8, 5, 6, 3, 2, F.relu, residual=True, n_out_heads=2, allow_zero_in_degree=True)
    GC.check_stack(model2, blocks, blocks[0].srcdata["feat"].cpu(), DEV)


def _losses(step, n=5):
    torch.manual_seed(0)
    out = []
    for _ in range(n):
        out.append(float(torch.as_tensor(step()).detach()))
    assert all(np.isfinite(v) for v in out) and out[-1] < out[0], out
    return out


def test_build_gatv2_full_batch_steps():
    wl = workloads.build_gatv2("cora", DEV, drop=False)
    _losses(lambda: wl.step()[0])
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in wl.model.parameters())


def test_build_gatv2_sampled_epochs():
    wl = workloads.build_gatv2("arxiv", DEV, scale=0.05, sampled=True, drop=False)
    assert wl.model.convs[0]._num_heads == 3 and wl.model.convs[0]._out_feats == 250 and len(wl.model.norms) == 2
    _losses(wl.epoch, 2)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in wl.model.parameters())


def test_gatv2_under_subgraph_steps():
    from bot_amd import minibatch
    wl = workloads.build_gatv2("cora", DEV, drop=False)
    ds, g = wl.dataset, wl.graph
    n = g.number_of_nodes()
    roles = minibatch.node_roles(n, ds.train_idx, ds.val_idx, ds.test_idx)
    g.ndata["feat"] = ds.feat
    sub = g.subgraph(torch.arange(0, n, 2, device=DEV))
    res = minibatch.subgraph_step(wl.model, sub, wl.optimizer, ds.labels, roles, step_kw=wl.step_kw)
    assert res is not None and np.isfinite(float(res[0].detach()))


# ------------------------------------------------------------------------------------------------ 5. errors
def test_error_paths():
    name, g = _graphs()[3]
    n, E = g.number_of_nodes(), g.number_of_edges()
    fs, attn = torch.randn(n, 2, 4, device=DEV), torch.randn(1, 2, 4, device=DEV)
    assert ops.gatv2_logits(g, fs, fs, attn).shape == (E, 2, 1)
    for bad, text in (((fs[:-1], fs, attn), f"({n - 1}, 2, 4)"), ((fs, fs[:, :1], attn), f"({n}, 1, 4)"), ((fs, fs, attn[0, :1]), "(1, 4)")):
        with pytest.raises(ValueError) as err:
            ops.gatv2_logits(g, *bad)
        assert text in str(err.value)
    with pytest.raises(DGLError, match="0-in-degree"):                # every fifth node of the graph has no in-edges
        bnn.GATv2Conv(4, 4, 2).to(DEV)(g, torch.randn(n, 4, device=DEV))
    out = bnn.GATv2Conv(4, 4, 2, allow_zero_in_degree=True).to(DEV)(g, torch.randn(n, 4, device=DEV))
    assert bool((out[g.in_degrees() == 0] == 0).all())
    part = BC.parent_graph(DEV, n=200, e_raw=1500, seed=7)
    part.halo = object()                                              # a partition's block carries a halo plan
    with pytest.raises(ValueError, match="partition"):
        ops.gatv2_logits(part, torch.randn(200, 1, 4, device=DEV), torch.randn(200, 1, 4, device=DEV), attn[:, :1])
    model = bnn.GATv2(8, 5, 6, 2, 2, F.relu).to(DEV)
    p = _parent()
    with pytest.raises(ValueError, match="edge_weight"):
        model(p, p.ndata["feat"], edge_weight=torch.ones(p.number_of_edges(), device=DEV))
    with pytest.raises(_C.BotKernelError, match="contiguous rows"):
        _C.gatv2_logits(g.csc, fs.transpose(1, 2), fs, attn[0], 0.2)
