"""DeeperGCN without a GPU: the tensor form of `ops.copy_u_softmax` against the float64 restatement (tests/gen_cases.py), gradcheck for x
and beta, the dbeta identity against a finite difference, the restated dx formula against autograd, `nn.GENConv` and `nn.DeeperGCN` on
CPU tensors over the emulated backend against their float64 restatements, parameters and state_dict keys, every error path,
`workloads.build_gen`, and the argument checks of the two new entry points.  tests/test_gen_gpu.py holds the kernels to the same
restatements."""
import inspect

import numpy as np
import pytest
import torch

import bot_amd
from bot_amd import nn as bnn
from bot_amd import ops, workloads
from tests import _oracle_backend
from tests import block_cases as BC
from tests import gen_cases as GC
from tests import sage_cases as SG


@pytest.fixture
def backend(monkeypatch):
    _oracle_backend.install(monkeypatch)


def _blocks(g, fanouts, n_seeds=150, seed=0):
    seeds = torch.randperm(g.number_of_nodes(), generator=torch.Generator().manual_seed(seed + 3))[:n_seeds]
    return BC.host_blocks(g, seeds, fanouts, seed)


# ------------------------------------------------------------------------------------------------ the op: tensor form
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("beta", [0.0, 0.1, 1.0, 10.0])
def test_tensor_form_against_fp64_restatement(relu, beta):
    g = SG.small_graph(65, 90, 7)
    indptr, indices = SG.csc_of(g)
    x = torch.randn(90, 7, generator=torch.Generator().manual_seed(1))
    res = GC.forward64(indptr, indices, x.numpy(), beta, relu, 1e-7)
    out = ops.copy_u_softmax(g, x.double(), beta, relu=relu, eps=1e-7)
    np.testing.assert_allclose(out.numpy(), res["out"], rtol=0, atol=1e-12)
    assert bool((out[torch.from_numpy(res["deg"] == 0)] == 0).all()) and int((res["deg"] == 0).sum()) >= 10
    out32 = ops.copy_u_softmax(g, x, torch.tensor([beta]), relu=relu, eps=1e-7, impl="tensor")
    np.testing.assert_allclose(out32.numpy(), res["out"], rtol=0, atol=1e-5)
    out3 = ops.copy_u_softmax(g, x.double().reshape(90, 7, 1).expand(90, 7, 2), beta, relu=relu, eps=1e-7)
    assert out3.shape == (65, 7, 2) and torch.equal(out3[:, :, 1], out)
    assert "copy_u_softmax" in ops.__all__ and ops.softmax_agg_default_impl in ops.SOFTMAX_AGG_IMPLS


def test_restatement_limits():
    """beta = 0 is the mean, a large beta the max, and q - out^2 is a variance: never negative."""
    g = SG.small_graph(64, 100, 3)
    indptr, indices = SG.csc_of(g)
    x = np.random.default_rng(0).standard_normal((100, 5)).astype(np.float32)
    deg = np.diff(indptr)
    mean = GC.forward64(indptr, indices, x, 0.0)
    want = np.zeros((64, 5))
    for r in range(64):
        if deg[r]:
            want[r] = x[indices[indptr[r]:indptr[r + 1]]].astype(np.float64).mean(0)
    np.testing.assert_allclose(mean["out"], want, rtol=0, atol=1e-13)
    big = GC.forward64(indptr, indices, x, 1e4)
    np.testing.assert_allclose(big["out"], SG.max_forward(indptr, indices, x)[0], rtol=0, atol=1e-12)
    mid = GC.forward64(indptr, indices, x, 1.3, True, 1e-7)
    assert np.all(mid["q"] - mid["out"] ** 2 >= -1e-12)
    xi = np.random.default_rng(1).integers(-8, 9, (100, 5)).astype(np.float32)
    for relu in (False, True):
        np.testing.assert_allclose(GC.mean32(indptr, indices, xi, relu), GC.forward64(indptr, indices, xi, 0.0, relu)["out"], rtol=2 ** -23, atol=0)


def test_gradcheck_of_the_tensor_form_for_x_and_beta():
    g = SG.small_graph(20, 30, 8)
    gen = torch.Generator().manual_seed(2)
    x = torch.randn(30, 4, dtype=torch.float64, generator=gen).requires_grad_()
    beta = torch.tensor([0.7], dtype=torch.float64, requires_grad=True)
    for relu in (False, True):
        assert torch.autograd.gradcheck(lambda a, b: ops.copy_u_softmax(g, a, b, relu=relu, eps=1e-7), (x, beta))


@pytest.mark.parametrize("relu", [False, True])
def test_restated_gradients_against_autograd_and_finite_difference(relu):
    """The two formulas the kernels implement - dx over the out-edges from (out, lse), dbeta = sum dout (q - out^2) - against autograd of
    the float64 tensor form, and dbeta also against a central finite difference of the restated forward."""
    g = SG.small_graph(40, 60, 9)
    indptr, indices = SG.csc_of(g)
    gen = torch.Generator().manual_seed(3)
    x = torch.randn(60, 6, dtype=torch.float64, generator=gen)
    x[::7] = 0.0                                                      # the ReLU's kink: gradient 0 there (torch's convention)
    dout = torch.randn(40, 6, dtype=torch.float64, generator=gen)
    beta, eps = 1.7, 1e-7
    xa = x.clone().requires_grad_()
    ba = torch.tensor([beta], dtype=torch.float64, requires_grad=True)
    ops.copy_u_softmax(g, xa, ba, relu=relu, eps=eps).backward(dout)
    res = GC.forward64(indptr, indices, x.numpy(), beta, relu, eps)
    dx, _ = GC.backward64(g.csr.indptr.numpy(), g.csr.indices.numpy(), x.numpy(), beta, relu, eps, dout.numpy(), res["out"], res["lse"], 0.0)
    np.testing.assert_allclose(dx, xa.grad.numpy(), rtol=0, atol=1e-12)
    np.testing.assert_allclose(GC.dbeta64(res, dout.numpy()), float(ba.grad), rtol=0, atol=1e-12)
    h = 1e-5
    fd = sum(s * float((GC.forward64(indptr, indices, x.numpy(), beta + s * h, relu, eps)["out"] * dout.numpy()).sum()) for s in (1, -1)) / (2 * h)
    np.testing.assert_allclose(GC.dbeta64(res, dout.numpy()), fd, rtol=0, atol=1e-7)


def test_impl_switch_and_beta_cache(monkeypatch):
    g = SG.small_graph(20, 30, 8)
    x = torch.randn(30, 4)
    with pytest.raises(ValueError, match="impl"):
        ops.copy_u_softmax(g, x, impl="triton")
    monkeypatch.setenv("BOT_SOFTMAX_AGG", "nothing")                  # read at call time
    with pytest.raises(ValueError, match="BOT_SOFTMAX_AGG"):
        ops.copy_u_softmax(g, x)
    monkeypatch.setenv("BOT_SOFTMAX_AGG", "tensor")
    assert ops.copy_u_softmax(g, x).shape == (20, 4)
    monkeypatch.delenv("BOT_SOFTMAX_AGG")
    with pytest.raises(bot_amd._C.BotKernelError):                    # no quiet fall-back: the kernel form refuses CPU tensors
        ops.copy_u_softmax(g, x, impl="kernel")
    a, b = ops._device_beta(0.25, x), ops._device_beta(0.25, x)
    assert a is b and a.dtype == torch.float32 and a.tolist() == [0.25] and ops._device_beta(0.5, x) is not a


def test_op_error_paths():
    g = SG.small_graph(20, 30, 8)
    with pytest.raises(ValueError, match="source nodes"):
        ops.copy_u_softmax(g, torch.randn(29, 4))
    with pytest.raises(ValueError, match="features"):
        ops.copy_u_softmax(g, torch.randn(30))
    with pytest.raises(ValueError, match="beta"):
        ops.copy_u_softmax(g, torch.randn(30, 4), torch.ones(2))
    with pytest.raises(ValueError, match="beta"):
        ops.copy_u_softmax(g, torch.randn(30, 4), torch.ones(1, dtype=torch.float64))
    part = BC.parent_graph("cpu", n=200, e_raw=1500, seed=7)
    part.halo = object()                                              # a partition's block carries a halo plan
    with pytest.raises(ValueError, match="partition"):
        ops.copy_u_softmax(part, torch.randn(200, 4))
    with pytest.raises(ValueError, match="partition"):
        bnn.GENConv(4, 4)(part, torch.randn(200, 4))


# ------------------------------------------------------------------------------------------------ GENConv
@pytest.mark.parametrize("kw", [dict(), dict(msg_norm=True, learn_msg_scale=True), dict(mlp_layers=2), dict(learn_beta=True, beta=0.5),
                                dict(mlp_layers=2, norm="layer", msg_norm=True), dict(mlp_layers=3, norm="none", learn_beta=True)])
@pytest.mark.parametrize("fin,fout", [(3, 16), (16, 3)])
def test_genconv_against_fp64_restatement(backend, kw, fin, fout):
    g = BC.parent_graph("cpu")
    GC.check_conv(g, "cpu", fin, fout, **kw)
    b = _blocks(g, (5,))[0]
    assert b.number_of_src_nodes() > b.number_of_dst_nodes()
    GC.check_conv(b, "cpu", fin, fout, seed=1, **kw)


def test_genconv_edge_features_isolated_destinations_and_feature_pairs(backend):
    g = SG.small_graph(65, 65, 10)                                    # every fifth node has no in-edges
    GC.check_conv(g, "cpu", 6, 4, learn_beta=True)
    GC.check_conv(g, "cpu", 6, 4, edge_feats=True, learn_beta=True, msg_norm=True)
    GC.check_conv(BC.parent_graph("cpu"), "cpu", 5, 5, edge_feats=True)
    b = SG.small_graph(30, 50, 11)
    conv = bnn.GENConv(5, 4).eval()
    hs, hd = torch.randn(50, 5), torch.randn(30, 5)
    src, dst, n_src, n_dst, _ = SG.edge_lists(b)
    ref = GC.gen_conv64(conv, src, dst, n_dst, hs.double(), hd.double(), {k: v.detach().double() for k, v in conv.named_parameters()})
    np.testing.assert_allclose(conv(b, (hs, hd)).detach().numpy(), ref.numpy(), rtol=0, atol=1e-4)
    with pytest.raises(ValueError, match="destination"):
        conv(b, (hs, hd[:-1]))
    with pytest.raises(ValueError, match="source nodes"):
        conv(b, hd)
    with pytest.raises(ValueError, match="features"):
        conv(b, torch.randn(50, 6))
    with pytest.raises(ValueError, match="edge_feats"):
        conv(b, hs, edge_feats=torch.randn(b.number_of_edges(), 4))


def test_genconv_parameters_state_dict_keys_and_error_paths():
    conv = bnn.GENConv(6, 4)
    assert set(conv.state_dict()) == {"mlp.0.weight", "mlp.0.bias"} and sum(p.numel() for p in conv.parameters()) == 6 * 4 + 4
    assert conv.beta == 1.0 and conv.eps == 1e-7 and conv.msg_scale is None
    conv = bnn.GENConv(6, 4, beta=0.5, learn_beta=True, msg_norm=True, mlp_layers=2)
    assert set(conv.state_dict()) == {"beta", "msg_scale", "mlp.0.weight", "mlp.0.bias", "mlp.1.weight", "mlp.1.bias", "mlp_norms.0.weight",
                                      "mlp_norms.0.bias", "mlp_norms.0.running_mean", "mlp_norms.0.running_var",
                                      "mlp_norms.0.num_batches_tracked"}
    assert sum(p.numel() for p in conv.parameters()) == 2 + (6 * 12 + 12) + 2 * 12 + (12 * 4 + 4)
    assert conv.beta.tolist() == [0.5] and conv.beta.requires_grad and not conv.msg_scale.requires_grad
    assert bnn.GENConv(6, 4, msg_norm=True, learn_msg_scale=True).msg_scale.requires_grad
    assert conv.mlp[0].weight.shape == (12, 6) and isinstance(conv.mlp_norms[0], torch.nn.BatchNorm1d)
    assert isinstance(bnn.GENConv(6, 4, mlp_layers=2, norm="layer").mlp_norms[0], torch.nn.LayerNorm)
    with pytest.raises(NotImplementedError, match="power"):
        bnn.GENConv(4, 4, aggregator="power")
    with pytest.raises(ValueError, match="aggregator"):
        bnn.GENConv(4, 4, aggregator="mean")
    with pytest.raises(ValueError, match="norm"):
        bnn.GENConv(4, 4, norm="group")
    with pytest.raises(ValueError, match="mlp_layers"):
        bnn.GENConv(4, 4, mlp_layers=0)
    assert {"GENConv", "DeeperGCN"} <= set(bnn.__all__)


# ------------------------------------------------------------------------------------------------ the stack, the recipe
@pytest.mark.parametrize("kw", [dict(), dict(learn_beta=True, msg_norm=True, mlp_layers=2, beta=0.5)])
def test_deepergcn_against_fp64_restatement(backend, kw):
    g = BC.parent_graph("cpu")
    torch.manual_seed(3)
    model = bnn.DeeperGCN(8, 5, 12, 3, dropout=0.5, **kw)
    assert len(model.convs) == len(model.norms) == 3 and model.node_encoder.weight.shape == (12, 8) and model.output.weight.shape == (5, 12)
    assert ("convs.2.beta" in model.state_dict()) == bool(kw)
    GC.check_stack(model, g, g.ndata["feat"], "cpu")
    blocks = _blocks(g, (4, 5, 6))
    GC.check_stack(bnn.DeeperGCN(8, 5, 12, 3, **kw), blocks, blocks[0].srcdata["feat"], "cpu")
    with pytest.raises(ValueError):
        model(blocks[:2])
    with pytest.raises(TypeError):
        model(g)
    with pytest.raises(ValueError):
        bnn.DeeperGCN(8, 5, 12, 0)


def test_deepergcn_parameter_count():
    model = bnn.DeeperGCN(8, 5, 12, 3, learn_beta=True)
    per_conv = 1 + 12 * 12 + 12
    assert sum(p.numel() for p in model.parameters()) == (8 * 12 + 12) + 3 * per_conv + 3 * 2 * 12 + (12 * 5 + 5)


@pytest.mark.parametrize("learn_beta", [True, False])
def test_build_gen_full_batch_step(backend, learn_beta):
    wl = workloads.build_gen("cora", "cpu", scale=0.25, learn_beta=learn_beta, drop=False)   # (the CPU emulation has no dropout stream)
    assert isinstance(wl.model, bnn.DeeperGCN) and len(wl.model.convs) == 2 and wl.model.convs[0]._out_feats == 16
    assert wl.dominant == ("spmm_softmax", (16, True, learn_beta)) and "DeeperGCN" in wl.describe
    res = wl.step()
    assert all(bool(torch.isfinite(torch.as_tensor(v)).all()) for v in res[3:6])
    params = dict(wl.model.named_parameters())
    assert ("convs.0.beta" in params) == learn_beta
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params.values())
    with pytest.raises(ValueError):
        workloads.build_gen("proteins", "cpu")


def test_build_gen_shapes():
    sig = inspect.signature(workloads.build_gen)
    assert [p for p in sig.parameters][:2] == ["name", "device"]
    assert {k: v.default for k, v in sig.parameters.items() if v.kind is v.KEYWORD_ONLY} == dict(
        sampled=False, scale=1.0, seed=0, drop=True, learn_beta=True)


# ------------------------------------------------------------------------------------------------ the C ABI's checks, no GPU
def test_argument_validation_without_gpu():
    from bot_amd import _C
    lib = _C._lib
    buf = torch.zeros(256)
    p = buf.data_ptr()
    assert p % 16 == 0
    ok_f = dict(n=4, nnz=0, indices=None, items=p, long_rows=None, long_ptr=None, n_long=0, n_slots=0, x=p + 64, ldx=4, F=4, beta=p + 128,
                eps=0.0, out=p + 192, ldo=4, lse=p + 256, ldl=4, q=None, ldq=4, ws=None)
    ok_b = dict(n=4, nnz=0, indices=None, items=p, long_rows=None, long_ptr=None, n_long=0, x=p + 64, ldx=4, beta=p + 128, eps=0.0,
                dout=None, ldd=4, out=None, ldo=4, lse=None, ldl=4, F=4, dx=p + 192, lddx=4, partial=None)

    def fwd(**k):
        a = dict(ok_f, **k)
        return lib.bot_spmm_softmax_f32(None, a["indices"], a["n"], a["nnz"], a["items"], 4, a["long_rows"], a["long_ptr"], a["n_long"], a["n_slots"],
                                        a["x"], a["ldx"], a["F"], a["beta"], 1, a["eps"], a["out"], a["ldo"], a["lse"], a["ldl"], a["q"], a["ldq"],
                                        a["ws"], None)

    def bwd(**k):
        a = dict(ok_b, **k)
        return lib.bot_spmm_softmax_bwd_f32(None, a["indices"], a["n"], a["nnz"], a["items"], 4, a["long_rows"], a["long_ptr"], a["n_long"], a["x"],
                                            a["ldx"], a["beta"], 1, a["eps"], a["dout"], a["ldd"], a["out"], a["ldo"], a["lse"], a["ldl"], a["F"],
                                            a["dx"], a["lddx"], a["partial"], None)
    err = lib.bot_last_error
    for f in (fwd, bwd):
        assert f(n=0) == 0 and f(n=0, items=None, x=None) == 0                                  # an empty problem is a no-op
        assert f(F=0) == -2 and b"F=0" in err()
        assert f(n=-1) == -2 and f(nnz=-1) == -2 and f(n_long=-1) == -2 and b"negative" in err()
        assert f(n=2 ** 31) == -2 and f(nnz=2 ** 31 - 1) == -2 and b"int32" in err()
        assert f(eps=float("nan")) == -2 and f(eps=float("inf")) == -2 and b"eps" in err()
        assert f(items=None) == -1 and f(x=None) == -1 and f(beta=None) == -1 and b"NULL" in err()
        assert f(nnz=3) == -1 and b"indices" in err()                                          # edges without their operands
        assert f(n_long=1, **({"n_slots": 2} if f is fwd else {})) == -1 and b"long rows" in err()
        assert f(ldx=3) == -2 and b"stride" in err()
        assert f(items=p + 4) == -3 and f(x=p + 66) == -3 and f(beta=p + 130) == -3 and b"misaligned" in err()
    assert fwd(n_slots=-1) == -2
    assert fwd(out=None) == -1 and fwd(lse=None) == -1
    assert fwd(n_long=1, n_slots=0, long_rows=p, long_ptr=p, ws=p) == -2 and b"slots" in err()
    assert fwd(ldo=3) == -2 and fwd(ldl=3) == -2 and fwd(q=p + 320, ldq=3) == -2 and b"stride" in err()
    assert fwd(n=0, q=None, ldq=0) == 0                                                         # (ldq is not read without q)
    assert fwd(out=p + 64) == -2 and fwd(lse=p + 64) == -2 and fwd(q=p + 64) == -2 and fwd(lse=p + 192) == -2 and fwd(q=p + 192) == -2 \
        and fwd(q=p + 256) == -2 and b"alias" in err()
    assert fwd(out=p + 194) == -3 and fwd(lse=p + 258) == -3 and fwd(q=p + 322) == -3
    assert fwd(n_long=1, n_slots=2, long_rows=p, long_ptr=p, ws=p + 8) == -3
    assert bwd(dx=None) == -1
    assert bwd(nnz=3, indices=p, dout=p, out=p) == -1 and bwd(nnz=3, indices=p, dout=p, lse=p) == -1
    assert bwd(ldd=3) == -2 and bwd(ldo=3) == -2 and bwd(ldl=3) == -2 and bwd(lddx=3) == -2 and b"stride" in err()
    assert bwd(dx=p + 64) == -2 and bwd(dx=p + 192, dout=p + 192) == -2 and bwd(dx=p + 192, out=p + 192) == -2 \
        and bwd(dx=p + 192, lse=p + 192) == -2 and b"alias" in err()
    assert bwd(dx=p + 194) == -3 and bwd(dout=p + 2) == -3 and bwd(out=p + 2) == -3 and bwd(lse=p + 2) == -3
    assert bwd(n_long=1, long_rows=p, long_ptr=p, partial=p + 8) == -3
    assert lib.bot_abi_version() == 19
