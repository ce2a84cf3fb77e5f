"""GraphSAGE without a GPU: `ops.copy_u_max`, the `fn.max` / `fn.mean` reducers, `nn.SAGEConv` and `nn.GraphSAGE` on CPU tensors over
the emulated backend plus the max sweep's stand-ins (tests/sage_cases.py), against the float64 restatements; parameters and
state_dict keys per aggregator, every error path, `workloads.build_sage`, the new symbols' argument checks, and two checks of the
restatement itself (against torch.amax over padded neighbour lists; gradient mass is conserved).  tests/test_sage_gpu.py holds the
kernels to the same restatements."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bot_amd
from bot_amd import function as fn
from bot_amd import nn as bnn
from bot_amd import ops, workloads
from bot_amd.errors import DGLError
from tests import _oracle_backend
from tests import block_cases as BC
from tests import sage_cases as SG
from tests.parity_cases import grad_close

KINDS = ("mean", "gcn", "pool")


@pytest.fixture
def backend(monkeypatch):
    _oracle_backend.install(monkeypatch)
    SG.install(monkeypatch)


def _blocks(g, fanouts, n_seeds=150, seed=0):
    seeds = torch.randperm(g.number_of_nodes(), generator=torch.Generator().manual_seed(seed + 3))[:n_seeds]
    return BC.host_blocks(g, seeds, fanouts, seed)


# ------------------------------------------------------------------------------------------------ the restatement itself
def test_restatement_max_against_torch_amax_over_padded_neighbour_lists():
    g = SG.small_graph(65, 90, 1)
    indptr, indices = SG.csc_of(g)
    x = np.random.default_rng(0).standard_normal((90, 7)).astype(np.float32)
    out, arg = SG.max_forward(indptr, indices, x)
    deg = np.diff(indptr)
    pad = torch.full((65, int(deg.max()), 7), -np.inf)
    for r in range(65):
        pad[r, :deg[r]] = torch.from_numpy(x[indices[indptr[r]:indptr[r + 1]]])
    want = torch.where(torch.from_numpy(deg > 0)[:, None], pad.amax(1), torch.zeros(()))
    assert np.array_equal(out, want.numpy())
    SG.check_arg(indptr, arg)
    assert np.all(arg[deg == 0] == -1) and np.all(arg[deg > 0] >= 0)
    got = x[indices[np.maximum(arg, 0)], np.arange(7)[None, :]]
    assert np.array_equal(got[deg > 0], out[deg > 0])
    # ties: the smallest position, -0.0 == +0.0; relu gates m <= 0
    t = SG.tie_values(90, 7, 2)
    o, a = SG.max_forward(indptr, indices, t)
    for r in np.nonzero(deg > 0)[0]:
        seg = t[indices[indptr[r]:indptr[r + 1]]]
        for f in range(7):
            assert a[r, f] == indptr[r] + min(k for k in range(len(seg)) if seg[k, f] == o[r, f])
    orl, arl = SG.max_forward(indptr, indices, t, relu=True)
    assert np.array_equal(orl, np.maximum(o, 0)) and np.array_equal(arl, np.where(o > 0, a, -1))


def test_restatement_backward_conserves_gradient_mass():
    g = SG.small_graph(64, 100, 3)
    indptr, indices = SG.csc_of(g)
    rng = np.random.default_rng(1)
    for relu in (False, True):
        _, arg = SG.max_forward(indptr, indices, SG.tie_values(100, 9, 4), relu)
        dout = rng.standard_normal((64, 9))
        dx = SG.max_backward(indices, 100, dout, arg)
        np.testing.assert_allclose(dx.sum(0), (dout * (arg >= 0)).sum(0), rtol=0, atol=1e-12)


def test_standins_agree_with_each_other():
    """The CSR-side stand-in (the kernel's definition) gives the scatter form of `max_backward`."""
    g = SG.small_graph(63, 80, 5)
    x = torch.from_numpy(SG.tie_values(80, 6, 6))
    out, arg = SG.spmm_max_standin(g.csc, x, relu=True)
    dout = torch.randn(63, 6, dtype=torch.float64)
    dx = SG.spmm_max_bwd_standin(g.csr, g.csr2csc, dout, arg)
    np.testing.assert_allclose(dx.numpy(), SG.max_backward(g.csc.indices.numpy(), 80, dout.numpy(), arg.numpy()), rtol=0, atol=1e-12)


# ------------------------------------------------------------------------------------------------ op and reducers
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("shape", [(5,), (41,), (3, 4)])
def test_copy_u_max_against_autograd_of_the_restatement(backend, relu, shape):
    g = SG.small_graph(65, 90, 7)
    src, dst, n_src, n_dst, pos_src = SG.edge_lists(g)
    gen = torch.Generator().manual_seed(1)
    x = torch.randn((n_src,) + shape, generator=gen).requires_grad_()
    out, arg = ops.copy_u_max(g, x, relu=relu, return_arg=True)
    assert out.shape == arg.shape == (n_dst,) + shape and arg.dtype == torch.int32 and not arg.requires_grad
    o_ref, a_ref = SG.max_forward(*SG.csc_of(g), x.detach().reshape(n_src, -1).numpy(), relu)
    assert np.array_equal(out.detach().reshape(n_dst, -1).numpy(), o_ref) and np.array_equal(arg.reshape(n_dst, -1).numpy(), a_ref)
    dout = torch.randn(out.shape, generator=gen)
    out.backward(dout)
    x64 = x.detach().double().reshape(n_src, -1).requires_grad_()
    SG.relu_max(src, dst, n_dst, x64, arg.reshape(n_dst, -1), pos_src).backward(dout.double().reshape(n_dst, -1))
    grad_close(x.grad.reshape(n_src, -1), x64.grad.numpy())
    assert ops.copy_u_max(g, x.detach()).shape == out.shape and "copy_u_max" in ops.__all__
    with pytest.raises(ValueError):
        ops.copy_u_max(g, torch.randn((n_src - 1,) + shape))


def test_the_csr_is_built_only_for_a_gradient(backend):
    g = SG.small_graph(20, 30, 8)
    ops.copy_u_max(g, torch.randn(30, 4))
    assert g._csr is None
    x = torch.randn(30, 4, requires_grad=True)
    ops.copy_u_max(g, x).sum().backward()
    assert g._csr is not None and x.grad is not None


def test_update_all_max_and_mean(backend):
    g = SG.small_graph(40, 40, 9)
    E = g.number_of_edges()
    x, w = torch.randn(40, 6), torch.rand(E, 1)
    g.ndata["h"], g.edata["w"] = x, w
    g.update_all(fn.copy_u("h", "m"), fn.max("m", "o"))
    assert torch.equal(g.ndata["o"], ops.copy_u_max(g, x))
    deg = g.in_degrees().float()
    inv = torch.where(deg > 0, 1 / deg.clamp(min=1), torch.zeros(()))[:, None]
    g.update_all(fn.copy_u("h", "m"), fn.mean("m", "o"))
    assert torch.equal(g.ndata["o"], ops.copy_u_sum(g, x) * inv) and bool((g.ndata["o"][deg == 0] == 0).all())
    g.update_all(fn.u_mul_e("h", "w", "m"), fn.mean("m", "o"))
    assert torch.equal(g.ndata["o"], ops.u_mul_e_sum(g, x, w) * inv)
    g.update_all(fn.copy_u("h", "m"), fn.sum("m", "o"))
    assert torch.equal(g.ndata["o"], ops.copy_u_sum(g, x))
    with pytest.raises(NotImplementedError, match="max"):
        g.update_all(fn.u_mul_e("h", "w", "m"), fn.max("m", "o"))
    with pytest.raises(NotImplementedError):
        g.update_all(fn.copy_e("w", "m"), fn.mean("m", "o"))
    with pytest.raises(NotImplementedError):
        g.update_all(fn.copy_u("h", "m"), fn.max("other", "o"))


# ------------------------------------------------------------------------------------------------ SAGEConv
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("fin,fout", [(3, 16), (16, 3), (41, 16)])
@pytest.mark.parametrize("weighted", [False, True])
def test_sageconv_against_fp64_restatement(backend, monkeypatch, kind, fin, fout, weighted):
    if kind == "pool" and weighted:
        g = BC.parent_graph("cpu")
        with pytest.raises(ValueError, match="pool"):
            bnn.SAGEConv(fin, fout, "pool")(g, torch.randn(g.number_of_nodes(), fin), edge_weight=torch.ones(g.number_of_edges()))
        return
    g = BC.parent_graph("cpu")
    SG.check_conv(g, "cpu", kind, fin, fout, weighted, monkeypatch)
    b = _blocks(g, (5,))[0]
    assert b.number_of_src_nodes() > b.number_of_dst_nodes()
    SG.check_conv(b, "cpu", kind, fin, fout, weighted, monkeypatch, seed=1)


@pytest.mark.parametrize("kind", KINDS)
def test_sageconv_on_isolated_destinations_and_feature_pairs(backend, monkeypatch, kind):
    g = SG.small_graph(65, 65, 10)                       # every fifth node has no in-edges
    SG.check_conv(g, "cpu", kind, 6, 4, False, monkeypatch)
    SG.check_conv(g, "cpu", kind, 4, 6, kind != "pool", monkeypatch)
    b = SG.small_graph(30, 50, 11)
    conv = bnn.SAGEConv((5, 5) if kind == "gcn" else (5, 7), 4, kind)
    hs, hd = torch.randn(50, 5), torch.randn(30, 5 if kind == "gcn" else 7)
    out = conv(b, (hs, hd))
    src, dst, n_src, n_dst, pos_src = SG.edge_lists(b)
    ref = SG.sage_conv(kind, src, dst, n_src, n_dst, hs.double(), hd.double(), {k: v.detach().double() for k, v in conv.state_dict().items()}, 4)
    np.testing.assert_allclose(out.detach().numpy(), ref.numpy(), rtol=0, atol=1e-4)
    with pytest.raises(ValueError, match="destination"):
        conv(b, (hs, hd[:-1]))


def test_sageconv_parameters_and_state_dict_keys():
    want = {"mean": {"fc_self", "fc_neigh"}, "gcn": {"fc_neigh"}, "pool": {"fc_pool", "fc_self", "fc_neigh"}}
    for kind, mods in want.items():
        for bias in (True, False):
            conv = bnn.SAGEConv((6, 6) if kind == "gcn" else (6, 9), 4, kind, bias=bias)
            keys = {m + ".weight" for m in mods} | ({m + ".bias" for m in mods} if bias else set())
            if kind == "pool":
                keys.add("fc_pool.bias")
            assert set(conv.state_dict()) == keys
            count = 6 * 4 + (4 if bias else 0)
            if kind != "gcn":
                count += 9 * 4 + (4 if bias else 0)
            if kind == "pool":
                count += 6 * 6 + 6
            assert sum(p.numel() for p in conv.parameters()) == count
            assert conv.fc_neigh.weight.shape == (4, 6)
    conv = bnn.SAGEConv(8, 8, "mean")
    bound = torch.nn.init.calculate_gain("relu") * (6.0 / 16) ** 0.5
    assert float(conv.fc_neigh.weight.detach().abs().max()) <= bound and float(conv.fc_neigh.weight.detach().abs().max()) > 0.5 * bound
    out = bnn.SAGEConv(3, 5, "mean", activation=F.relu, norm=lambda t: t * 2.0, feat_drop=0.0)
    assert out.activation is F.relu


def test_sageconv_error_paths(backend):
    with pytest.raises(NotImplementedError, match="lstm"):
        bnn.SAGEConv(4, 4, "lstm")
    with pytest.raises(DGLError):
        bnn.SAGEConv(4, 4, "sum")
    with pytest.raises(DGLError, match="gcn"):
        bnn.SAGEConv((4, 5), 4, "gcn")
    g = BC.parent_graph("cpu")
    n, E = g.number_of_nodes(), g.number_of_edges()
    with pytest.raises(ValueError, match="pool"):
        bnn.SAGEConv(4, 4, "pool")(g, torch.randn(n, 4), edge_weight=torch.ones(E))
    with pytest.raises(DGLError):
        bnn.SAGEConv(4, 4, "mean")(g, torch.randn(n, 4), edge_weight=torch.ones(E - 1))
    with pytest.raises(DGLError):
        bnn.SAGEConv(4, 4, "mean")(g, torch.randn(n, 4), edge_weight=torch.ones(E, dtype=torch.float64))
    b = _blocks(g, (5,))[0]
    with pytest.raises(ValueError, match="source nodes"):
        bnn.SAGEConv(4, 4, "mean")(b, torch.randn(b.number_of_dst_nodes(), 4))
    part = BC.parent_graph("cpu", n=200, e_raw=1500, seed=7)
    part.halo = object()                                             # a partition's block carries a halo plan
    for kind in KINDS:
        with pytest.raises(ValueError, match="partition"):
            bnn.SAGEConv(4, 4, kind)(part, torch.randn(200, 4))


def test_activation_then_norm(backend):
    g = BC.parent_graph("cpu")
    x = torch.randn(g.number_of_nodes(), 4)
    torch.manual_seed(0)
    plain = bnn.SAGEConv(4, 6, "mean")
    both = bnn.SAGEConv(4, 6, "mean", activation=F.relu, norm=lambda t: t - 1.0)
    both.load_state_dict(plain.state_dict())
    assert torch.equal(both(g, x), F.relu(plain(g, x)) - 1.0)


# ------------------------------------------------------------------------------------------------ the stack, the recipe
@pytest.mark.parametrize("kind", KINDS)
def test_graphsage_stack_against_fp64_restatement(backend, monkeypatch, kind):
    g = BC.parent_graph("cpu")
    torch.manual_seed(3)
    model = bnn.GraphSAGE(8, 5, 12, 3, F.relu, aggregator_type=kind, norm="batch", dropout=0.5)
    assert [k for k in model.state_dict() if k.startswith("norms.0")] and len(model.norms) == 2
    SG.check_stack(model, g, g.ndata["feat"], "cpu", monkeypatch)
    blocks = _blocks(g, (4, 5, 6))
    model2 = bnn.GraphSAGE(8, 5, 12, 3, F.relu, aggregator_type=kind, norm="none")
    SG.check_stack(model2, blocks, blocks[0].srcdata["feat"], "cpu", monkeypatch)
    if kind != "pool":
        ews = [0.5 + torch.rand(b.number_of_edges()) for b in blocks]
        SG.check_stack(model2, blocks, blocks[0].srcdata["feat"], "cpu", monkeypatch, edge_weight=ews)
        SG.check_stack(model, g, g.ndata["feat"], "cpu", monkeypatch, edge_weight=0.5 + torch.rand(g.number_of_edges()))
    with pytest.raises(ValueError):
        model2(blocks[:2])
    with pytest.raises(ValueError):
        model2(blocks, edge_weight=torch.ones(3))
    with pytest.raises(ValueError):
        model(g, g.ndata["feat"], edge_weight=[torch.ones(1)])
    with pytest.raises(TypeError):
        model(g)


@pytest.mark.parametrize("aggregator", ["mean", "pool"])
def test_build_sage_full_batch_step(backend, aggregator):
    wl = workloads.build_sage("cora", "cpu", aggregator=aggregator, scale=0.25)
    assert isinstance(wl.model, bnn.GraphSAGE) and len(wl.model.convs) == 2 and len(wl.model.norms) == 0
    assert wl.model.convs[0]._out_feats == 16 and aggregator in wl.describe
    res = wl.step()
    assert all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in res[3:6])
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in wl.model.parameters())
    with pytest.raises(ValueError):
        workloads.build_sage("proteins", "cpu")


def test_build_sage_shapes():
    import inspect
    sig = inspect.signature(workloads.build_sage)
    assert [p for p in sig.parameters][:2] == ["name", "device"]
    assert {k: v.default for k, v in sig.parameters.items() if v.kind is v.KEYWORD_ONLY} == dict(
        aggregator="mean", sampled=False, scale=1.0, seed=0, drop=True)


# ------------------------------------------------------------------------------------------------ the C ABI's checks, no GPU
def test_argument_validation_without_gpu():
    from bot_amd import _C
    lib = _C._lib
    fwd = lambda **k: lib.bot_spmm_max_f32(None, None, k.get("n", 4), 0, k.get("items"), 4, None, None, 0, 0, k.get("x"), k.get("ldx", 4),
                                           k.get("F", 4), 0, k.get("out"), 4, k.get("arg"), 4, None, None)
    bwd = lambda **k: lib.bot_spmm_max_bwd_f32(None, None, k.get("n", 4), 0, None, 4, None, None, 0, None, None, k.get("ldd", 4), None, 4,
                                               k.get("F", 4), None, 4, None, None)
    assert fwd(F=0) == -2 and b"F=0" in lib.bot_last_error()
    assert fwd(n=-1) == -2
    assert fwd() == -1 and b"NULL" in lib.bot_last_error()
    assert fwd(n=0) == 0                                               # an empty problem is a no-op
    assert bwd(F=0) == -2 and bwd(n=-1) == -2 and bwd() == -1 and bwd(n=0) == 0
    buf = torch.zeros(64)
    p = buf.data_ptr()
    assert fwd(items=p, x=p, out=p + 16, arg=p + 32, ldx=3) == -2 and b"stride" in lib.bot_last_error()
    assert fwd(items=p, x=p, out=p, arg=p + 32) == -2 and b"alias" in lib.bot_last_error()
    assert lib.bot_abi_version() == 19
