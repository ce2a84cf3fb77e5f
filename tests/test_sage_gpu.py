"""GraphSAGE on the MI355X: the max sweep pair (csrc/spmm_max.hip) against the numpy restatement (tests/sage_cases.py) entry for entry -
a max does not round, and the backward's integer-valued sums are exact - `ops.copy_u_max` and the `fn.max` / `fn.mean` reducers,
`nn.SAGEConv` and `nn.GraphSAGE` against their float64 restatements under the suite's own criteria (tests/parity_cases.py), and one
train step / one sampled epoch of `workloads.build_sage`."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bot_amd
from bot_amd import _C, ops, workloads
from bot_amd import function as fn
from bot_amd import nn as bnn
from bot_amd.sampling import MultiLayerNeighborSampler, NodeDataLoader, sample_block
from tests import block_cases as BC
from tests import sage_cases as SG
from tests.parity_cases import grad_close

pytestmark = pytest.mark.gpu
DEV = "cuda"
WIDTHS = (1, 3, 4, 5, 40, 64, 65, 256, 1000)     # every lane width and group size; 1000 walks feature tiles
KINDS = ("mean", "gcn", "pool")


@functools.lru_cache(maxsize=None)
def _graphs():
    """(name, graph on the device) of the kernel tests: 1 / 63 / 64 / 65 rows with isolated rows and parallel edges, with the default
    chunk and with chunk = 4 (long rows: the chunk and combine kernels), and a block with n_src > n_dst."""
    out = []
    for n in (1, 63, 64, 65):
        out.append((f"square{n}", SG.small_graph(n, n, n).to(DEV)))
    out.append(("long65", SG.small_graph(65, 65, 70, chunk=4).to(DEV)))
    out.append(("block", SG.small_graph(63, 200, 71).to(DEV)))
    out.append(("longblock", SG.small_graph(64, 130, 72, chunk=4).to(DEV)))
    assert out[4][1].csc.n_long > 0 and out[4][1].csr.n_long > 0 and out[0][1].csc.n_long == 0
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _hub():
    """tests.test_subgraph_gpu._hub_graph(): hub rows above 2 048 in-edges, so the chunks and the combine run at the default chunk; with
    its values and the restatement's (out, arg) for relu off and on, computed once."""
    from tests.test_subgraph_gpu import _hub_graph
    g = _hub_graph()
    indptr, indices = SG.csc_of(g)
    assert int(np.diff(indptr).max()) > 2048 and g.csc.n_long > 0 and g.csr.n_long > 0
    x = SG.tie_values(g.number_of_nodes(), 40, 5)
    return g, x, {relu: SG.max_forward(indptr, indices, x, relu) for relu in (False, True)}


def _slab(a, pad, dev=DEV):
    """A [n, F] device view of `a` inside a [n, F + pad] buffer (row stride F + pad)."""
    t = torch.from_numpy(a)
    buf = torch.full((t.shape[0], t.shape[1] + pad), 7, dtype=t.dtype).to(dev)
    view = buf[:, :t.shape[1]]
    view.copy_(t.to(dev))
    return view


def _same_bytes(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ 1. forward, exact
@pytest.mark.parametrize("F_", WIDTHS)
def test_max_forward_is_exact(F_):
    for name, g in _graphs():
        indptr, indices = SG.csc_of(g)
        x = SG.tie_values(g.number_of_src_nodes(), F_, 3 * F_ + len(name))
        for relu in (False, True):
            want_out, want_arg = SG.max_forward(indptr, indices, x, relu)
            for pad in (0, 3, 4):                     # contiguous; an odd row stride (4-byte lanes); a strided slab that keeps wide lanes
                xd = _slab(x, pad)
                n = g.number_of_dst_nodes()
                out = torch.full((n, F_ + pad), 9.0, device=DEV)[:, :F_] if pad else None
                arg = torch.full((n, F_ + pad), 9, dtype=torch.int32, device=DEV)[:, :F_] if pad else None
                o, a = _C.spmm_max(g.csc, xd, relu, out=out, arg=arg)
                assert np.array_equal(o.cpu().numpy(), want_out), (name, F_, relu, pad)
                assert np.array_equal(a.cpu().numpy(), want_arg), (name, F_, relu, pad)
                if pad:
                    assert o.data_ptr() == out.data_ptr() and a.data_ptr() == arg.data_ptr()
                    assert bool((o._base[:, F_:] == 9.0).all()) and bool((a._base[:, F_:] == 9).all())     # nothing beyond the row
                o2, a2 = _C.spmm_max(g.csc, xd, relu)
                assert _same_bytes(o2, o) and torch.equal(a2, a)
        assert "spmm_max_kernel" in _C._lib.bot_last_kernel().decode()


def test_max_forward_on_the_hub_graph_is_exact():
    g, x, want = _hub()
    xd = torch.from_numpy(x).to(DEV)
    for relu in (False, True):
        o, a = _C.spmm_max(g.csc, xd, relu)
        assert np.array_equal(o.cpu().numpy(), want[relu][0]) and np.array_equal(a.cpu().numpy(), want[relu][1])
        o2, a2 = _C.spmm_max(g.csc, xd, relu)
        assert _same_bytes(o2, o) and torch.equal(a2, a)


def test_max_forward_with_nan_and_inf_stays_inside_the_row():
    name, g = _graphs()[4]
    indptr, indices = SG.csc_of(g)
    x = SG.tie_values(g.number_of_src_nodes(), 12, 1)
    x[::3, ::2] = np.nan
    x[1::3, 1::2] = -np.inf
    for relu in (False, True):
        o, a = _C.spmm_max(g.csc, torch.from_numpy(x).to(DEV), relu)
        torch.cuda.synchronize()
        SG.check_arg(indptr, a.cpu().numpy())
    clean = np.where(np.isnan(x), np.float32(-np.inf), x)              # -inf is an ordinary value: a row of -inf has a position
    o, a = _C.spmm_max(g.csc, torch.from_numpy(clean).to(DEV), False)
    want_out, want_arg = SG.max_forward(indptr, indices, clean, False)
    assert np.array_equal(o.cpu().numpy(), want_out) and np.array_equal(a.cpu().numpy(), want_arg)


# ------------------------------------------------------------------------------------------------ 2. backward, exact
def _check_backward(g, arg, F_, seed, pad=0):
    rng = np.random.default_rng(seed)
    n_dst, n_src = g.number_of_dst_nodes(), g.number_of_src_nodes()
    dout = rng.integers(-8, 9, (n_dst, F_)).astype(np.float32)           # every float32 sum is exact
    want = SG.max_backward(g.csc.indices.cpu().numpy(), n_src, dout, arg)
    dd, ad = _slab(dout, pad), _slab(arg, pad)
    out = torch.full((n_src, F_ + pad), 9.0, device=DEV)[:, :F_] if pad else None
    dx = _C.spmm_max_bwd(g.csr, g.csr2csc, dd, ad, out=out)
    got = dx.cpu().double().numpy()
    assert np.array_equal(got, want)
    assert np.array_equal(got.sum(0), (dout.astype(np.float64) * (arg >= 0)).sum(0))      # every column's gradient mass is conserved
    if pad:
        assert bool((dx._base[:, F_:] == 9.0).all())
    assert _same_bytes(_C.spmm_max_bwd(g.csr, g.csr2csc, dd, ad), dx)


@pytest.mark.parametrize("F_", WIDTHS)
def test_max_backward_is_exact(F_):
    for name, g in _graphs():
        indptr, indices = SG.csc_of(g)
        x = SG.tie_values(g.number_of_src_nodes(), F_, 5 * F_ + len(name))
        for relu in (False, True):
            _, arg = SG.max_forward(indptr, indices, x, relu)
            for pad in (0, 3, 4):
                _check_backward(g, arg, F_, F_ + pad, pad)
        assert "spmm_max_bwd_kernel" in _C._lib.bot_last_kernel().decode()


def test_max_sweeps_on_the_edge_case_graph_at_32_lanes():
    """The one group width WIDTHS leaves out (17 columns of 4-byte lanes: groups of 32), forward and backward, on SG.sweep_edges: with
    chunk = 8 its rows above 8 in-edges run as chunks of a long row, with chunk = 128 the rows of 63 / 64 / 65 in-edges are walked
    whole, 32 ids at a time (full batches of four, their tails, a second and a third group of ids)."""
    F_ = 17
    src, dst, n = SG.sweep_edges()
    for chunk in (8, 128):
        g = bot_amd.Graph(src, dst, n, chunk=chunk).to(DEV)
        assert (g.csc.n_long > 0 and g.csr.n_long > 0) == (chunk == 8)
        indptr, indices = SG.csc_of(g)
        x = SG.tie_values(n, F_, 23)
        for relu in (False, True):
            want_out, want_arg = SG.max_forward(indptr, indices, x, relu)
            o, a = _C.spmm_max(g.csc, torch.from_numpy(x).to(DEV), relu)
            assert _C._lib.bot_last_kernel().decode() == "bot::spmm_max_kernel<1,32,1>"
            assert np.array_equal(o.cpu().numpy(), want_out) and np.array_equal(a.cpu().numpy(), want_arg), (chunk, relu)
            _check_backward(g, want_arg, F_, 29 + relu)
            assert _C._lib.bot_last_kernel().decode() == "bot::spmm_max_bwd_kernel<1,32,1>"


def test_max_backward_on_the_hub_graph_is_exact():
    g, x, want = _hub()
    for relu in (False, True):
        _check_backward(g, want[relu][1], 40, 17)


# ------------------------------------------------------------------------------------------------ 3. op and reducers
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", [(5,), (41,), (64,), (3, 4)])
def test_copy_u_max_against_autograd_of_the_restatement(relu, shape):
    for name, g in (_graphs()[3], _graphs()[5], _graphs()[6]):
        src, dst, n_src, n_dst, pos_src = SG.edge_lists(g)
        gen = torch.Generator().manual_seed(1)
        x = torch.randn((n_src,) + shape, generator=gen).to(DEV).requires_grad_()
        out, arg = ops.copy_u_max(g, x, relu=relu, return_arg=True)
        assert out.shape == arg.shape == (n_dst,) + shape and arg.dtype == torch.int32 and not arg.requires_grad
        o_ref, a_ref = SG.max_forward(*SG.csc_of(g), x.detach().cpu().reshape(n_src, -1).numpy(), relu)
        assert np.array_equal(out.detach().cpu().reshape(n_dst, -1).numpy(), o_ref)
        assert np.array_equal(arg.cpu().reshape(n_dst, -1).numpy(), a_ref)
        dout = torch.randn(out.shape, generator=gen)
        out.backward(dout.to(DEV))
        x64 = x.detach().cpu().double().reshape(n_src, -1).requires_grad_()
        SG.relu_max(src, dst, n_dst, x64, arg.cpu().reshape(n_dst, -1), pos_src).backward(dout.double().reshape(n_dst, -1))
        grad_close(x.grad.reshape(n_src, -1), x64.grad.numpy())


def test_update_all_max_and_mean():
    name, g = _graphs()[3]
    n, E = g.number_of_nodes(), g.number_of_edges()
    x, w = torch.randn(n, 6, device=DEV), torch.rand(E, 1, device=DEV)
    g.ndata["h"], g.edata["w"] = x, w
    g.update_all(fn.copy_u("h", "m"), fn.max("m", "o"))
    assert torch.equal(g.ndata["o"], ops.copy_u_max(g, x))
    deg = g.in_degrees().float()
    inv = torch.where(deg > 0, 1 / deg.clamp(min=1), torch.zeros((), device=DEV))[:, None]
    g.update_all(fn.copy_u("h", "m"), fn.mean("m", "o"))
    assert torch.equal(g.ndata["o"], ops.copy_u_sum(g, x) * inv) and bool((g.ndata["o"][deg == 0] == 0).all())
    g.update_all(fn.u_mul_e("h", "w", "m"), fn.mean("m", "o"))
    assert torch.equal(g.ndata["o"], ops.u_mul_e_sum(g, x, w) * inv)
    with pytest.raises(NotImplementedError, match="max"):
        g.update_all(fn.u_mul_e("h", "w", "m"), fn.max("m", "o"))


# ------------------------------------------------------------------------------------------------ 4. SAGEConv
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


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fin,fout", [(3, 16), (16, 3), (41, 16)])
@pytest.mark.parametrize("weighted", [False, True])
def test_sageconv_against_fp64_restatement(monkeypatch, kind, fin, fout, weighted):
    if kind == "pool" and weighted:
        g = _parent()
        with pytest.raises(ValueError, match="pool"):
            bnn.SAGEConv(fin, fout, "pool").to(DEV)(g, torch.randn(g.number_of_nodes(), fin, device=DEV),
                                                    edge_weight=torch.ones(g.number_of_edges(), device=DEV))
        return
    SG.check_conv(_parent(), DEV, kind, fin, fout, weighted, monkeypatch)
    SG.check_conv(_block(), DEV, kind, fin, fout, weighted, monkeypatch, seed=1)


@pytest.mark.parametrize("kind", KINDS)
def test_sageconv_on_isolated_destinations(monkeypatch, kind):
    SG.check_conv(_graphs()[3][1], DEV, kind, 6, 4, False, monkeypatch)
    SG.check_conv(_graphs()[3][1], DEV, kind, 4, 6, kind != "pool", monkeypatch)


# ------------------------------------------------------------------------------------------------ 5. stack and step
@pytest.mark.parametrize("kind", KINDS)
def test_graphsage_stack_against_fp64_restatement(monkeypatch, kind):
    g = _parent()
    torch.manual_seed(3)
    model = bnn.GraphSAGE(8, 5, 12, 3, F.relu, aggregator_type=kind, norm="batch", dropout=0.5)
    SG.check_stack(model, g, g.ndata["feat"].cpu(), DEV, monkeypatch)
    nids = torch.randperm(g.number_of_nodes(), generator=torch.Generator().manual_seed(3))[:600]
    _, _, blocks = next(iter(NodeDataLoader(g, nids, MultiLayerNeighborSampler([5, 7, 9]), batch_size=600, seed=4)))
    model2 = bnn.GraphSAGE(8, 5, 12, 3, F.relu, aggregator_type=kind, norm="none")
    SG.check_stack(model2, blocks, blocks[0].srcdata["feat"].cpu(), DEV, monkeypatch)
    if kind != "pool":
        gen = torch.Generator().manual_seed(5)
        ews = [(0.5 + torch.rand(b.number_of_edges(), generator=gen)).to(DEV) for b in blocks]
        SG.check_stack(model2, blocks, blocks[0].srcdata["feat"].cpu(), DEV, monkeypatch, edge_weight=ews)


@pytest.mark.parametrize("aggregator", ["pool", "mean"])
def test_build_sage_full_batch_step(aggregator):
    wl = workloads.build_sage("cora", DEV, aggregator=aggregator, scale=0.25)
    res = wl.step()
    assert all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in res[3:6])
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in wl.model.parameters())


@pytest.mark.parametrize("aggregator", ["pool", "mean"])
def test_build_sage_sampled_epoch(aggregator):
    wl = workloads.build_sage("cora", DEV, aggregator=aggregator, sampled=True, scale=0.25)
    assert len(wl.loader) == workloads.SAMPLED["cora"][1]
    loss = wl.epoch()
    assert np.isfinite(float(loss))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in wl.model.parameters())
