"""DeeperGCN with raw edge features without a GPU: the float64 restatement (tests/gen_edge_cases.py) against float64 autograd, the tensor form
of `ops.u_add_e_softmax` against it, gradcheck for x, weight, bias and beta, the dbias identity, the non-vacuity of the derived bounds
(three wrong restatements must exceed them), `nn.GENConv(edge_dim=)` and `nn.DeeperGCN(edge_dim=)` on CPU tensors over the emulated backend
against their float64 restatements, state_dict keys, every refusal, `workloads.build_gen_edge`, and the argument checks of the two new
entry points.  tests/test_gen_edge_gpu.py holds the kernels to the same restatements."""
import inspect

import numpy as np
import pytest
import torch

from bot_amd import nn as bnn
from bot_amd import ops, workloads
from tests import _oracle_backend
from tests import block_cases as BC
from tests import gen_cases as GC
from tests import gen_edge_cases as GE
from tests import sage_cases as SG

EXP_ERR = 4 * GC.U          # the ceiling tests/test_gen_gpu.py asserts for the kernels' exponential; no kernel runs here


@pytest.fixture
def backend(monkeypatch):
    _oracle_backend.install(monkeypatch)


def _inputs(g, F, K, seed, bias=True):
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(g.number_of_src_nodes(), F, generator=gen)
    ef = torch.randn(g.number_of_edges(), K, generator=gen)
    w = torch.randn(F, K, generator=gen) / K ** 0.5
    b = torch.randn(F, generator=gen) if bias else None
    dout = torch.randn(g.number_of_dst_nodes(), F, generator=gen)
    return x, ef, w, b, dout


def _autograd64(arrays, x, ef, w, b, beta, relu, eps, dout):
    """out and the four gradients by float64 autograd over `gen_cases.softmax_agg64` (edge-list form)."""
    src, dst, n_src, n_dst = torch.from_numpy(arrays[0]), torch.from_numpy(arrays[1]), arrays[2], arrays[3]
    xs, ws, bs = x.double().requires_grad_(), w.double().requires_grad_(), b.double().requires_grad_()
    bt = torch.tensor(float(beta), dtype=torch.float64, requires_grad=True)
    z = xs[src] + (ef.double() @ ws.t() + bs)
    m = torch.relu(z) + eps if relu else z
    out = GC.softmax_agg64(src, dst, n_dst, m, bt)
    out.backward(dout.double())
    return out.detach().numpy(), xs.grad.numpy(), ws.grad.numpy(), bs.grad.numpy(), float(bt.grad)


# ------------------------------------------------------------------------------------------------ the restatement and the tensor form
@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("beta", [0.0, 0.1, 1.0, 10.0])
def test_restatement_and_tensor_form_against_fp64_autograd(relu, beta):
    g = SG.small_graph(65, 90, 7)
    assert not np.array_equal(g.csc.eid.numpy(), np.arange(g.number_of_edges()))
    arrays = GE.arrays_of(g)
    x, ef, w, b, dout = _inputs(g, 7, 3, 1)
    out, dx, dw, db, dbeta = _autograd64(arrays, x, ef, w, b, beta, relu, 1e-7, dout)
    res = GE.forward64(arrays, x.numpy(), ef.numpy(), w.numpy(), b.numpy(), beta, relu, 1e-7)
    np.testing.assert_allclose(res["out"], out, rtol=0, atol=1e-12)
    assert int((res["deg"] == 0).sum()) >= 10 and not res["out"][res["deg"] == 0].any()
    # the backward restatement from float64 operands (its operands are the kernel's float32 out and lse on the GPU)
    grads, _ = GE.backward64(arrays, x.numpy(), ef.numpy(), w.numpy(), b.numpy(), beta, relu, 1e-7, dout.numpy(), res["out"], res["lse"], 0.0)
    np.testing.assert_allclose(grads["dx"], dx, rtol=0, atol=1e-11)
    np.testing.assert_allclose(grads["dweight"], dw, rtol=0, atol=1e-10)
    np.testing.assert_allclose(grads["dbias"], db, rtol=0, atol=1e-10)
    np.testing.assert_allclose(grads["dbias"], grads["dx"].sum(0), rtol=0, atol=1e-10)          # dbias = the column sum of dx
    assert abs(GE.dbeta64(res, dout.numpy()) - dbeta) <= 1e-10 * max(1.0, abs(dbeta))
    # the op on CPU tensors runs the tensor form: float64 and float32
    xs, ws, bs = x.double().requires_grad_(), w.double().requires_grad_(), b.double().requires_grad_()
    bt = torch.tensor([beta], dtype=torch.float64, requires_grad=True)
    o64 = ops.u_add_e_softmax(g, xs, ef.double(), ws, bs, bt, relu=relu, eps=1e-7)
    o64.backward(dout.double())
    np.testing.assert_allclose(o64.detach().numpy(), out, rtol=0, atol=1e-12)
    np.testing.assert_allclose(xs.grad.numpy(), dx, rtol=0, atol=1e-11)
    np.testing.assert_allclose(ws.grad.numpy(), dw, rtol=0, atol=1e-10)
    np.testing.assert_allclose(bs.grad.numpy(), db, rtol=0, atol=1e-10)
    np.testing.assert_allclose(bs.grad.numpy(), xs.grad.numpy().sum(0), rtol=0, atol=1e-10)
    assert abs(float(bt.grad) - dbeta) <= 1e-10 * max(1.0, abs(dbeta))
    o32 = ops.u_add_e_softmax(g, x, ef, w, b, torch.tensor([beta]), relu=relu, eps=1e-7, impl="tensor")
    np.testing.assert_allclose(o32.numpy(), out, rtol=0, atol=2e-5)
    assert "u_add_e_softmax" in ops.__all__


def test_without_bias_and_on_a_block():
    """bias=None, and a block-shaped graph (n_src > n_dst)."""
    g = SG.small_graph(40, 130, 9)
    arrays = GE.arrays_of(g)
    x, ef, w, _, _ = _inputs(g, 5, 8, 2, bias=False)
    res = GE.forward64(arrays, x.numpy(), ef.numpy(), w.numpy(), None, 0.7, True, 1e-7)
    out = ops.u_add_e_softmax(g, x.double(), ef.double(), w.double(), None, 0.7, relu=True, eps=1e-7)
    np.testing.assert_allclose(out.numpy(), res["out"], rtol=0, atol=1e-12)


@pytest.mark.parametrize("relu", [False, True])
def test_gradcheck(relu):
    g = SG.small_graph(12, 20, 5)
    gen = torch.Generator().manual_seed(0)
    x = torch.randn(20, 3, dtype=torch.float64, generator=gen).requires_grad_()
    ef = torch.randn(g.number_of_edges(), 2, dtype=torch.float64, generator=gen)
    w = torch.randn(3, 2, dtype=torch.float64, generator=gen).requires_grad_()
    b = torch.randn(3, dtype=torch.float64, generator=gen).requires_grad_()
    beta = torch.tensor([0.8], dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(lambda x_, w_, b_, t_: ops.u_add_e_softmax(g, x_, ef, w_, b_, t_, relu=relu, eps=1e-7), (x, w, b, beta))


# ------------------------------------------------------------------------------------------------ the bounds bite
def _ratios(arrays, x, ef, w, b, beta, relu, wrong):
    """The largest |wrong - right| / bound per output, where `wrong` = (ef, w, b) of a wrong restatement."""
    args = (x.numpy(), beta, relu, 1e-7)
    right = GE.forward64(arrays, args[0], ef.numpy(), w.numpy(), b.numpy(), *args[1:])
    tol = GE.forward_bounds(right, beta, EXP_ERR)
    dout = torch.randn(right["out"].shape, generator=torch.Generator().manual_seed(5)).numpy()
    o32, l32 = right["out"].astype(np.float32), right["lse"].astype(np.float32)
    g_right, g_tol = GE.backward64(arrays, args[0], ef.numpy(), w.numpy(), b.numpy(), beta, relu, 1e-7, dout, o32, l32, EXP_ERR)
    wef, ww, wb = wrong
    bad = GE.forward64(arrays, args[0], wef, ww, wb, *args[1:])
    g_bad, _ = GE.backward64(arrays, args[0], wef, ww, wb, beta, relu, 1e-7, dout, o32, l32, EXP_ERR)
    some = right["deg"] > 0
    r = {k: float((np.abs(bad[k] - right[k])[some] / tol[k][some]).max()) for k in ("out", "lse", "q")}
    for k in ("dx", "dweight", "dbias"):
        ok = g_tol[k] > 0
        r[k] = float((np.abs(g_bad[k] - g_right[k])[ok] / g_tol[k][ok]).max())
    return r


@pytest.mark.parametrize("relu", [False, True])
@pytest.mark.parametrize("beta", [0.1, 1.0, 10.0])
def test_bounds_are_not_vacuous(relu, beta):
    """Each of three wrong restatements exceeds every bound on the test's own inputs: ef rows left in CSC position order where edge-id
    order is meant (on a graph whose csc.eid is not the identity), the bias dropped, weight indexed [j, f]."""
    g = SG.small_graph(65, 90, 7)
    arrays = GE.arrays_of(g)
    eid = arrays[5]
    assert not np.array_equal(eid, np.arange(len(eid)))
    x, ef, w, b, _ = _inputs(g, 6, 3, 3)
    wrongs = {"ef in position order": (ef.numpy()[np.argsort(eid)], w.numpy(), b.numpy()),
              "bias dropped": (ef.numpy(), w.numpy(), None),
              "weight indexed [j, f]": (ef.numpy(), np.ascontiguousarray(w.numpy().reshape(3, 6).T), b.numpy())}
    for name, wrong in wrongs.items():
        r = _ratios(arrays, x, ef, w, b, beta, relu, wrong)
        print(f"{name}: error / bound = " + ", ".join(f"{k} {v:.3g}" for k, v in r.items()))
        assert all(v > 1.0 for v in r.values()), (name, r)
    # and the right restatement sits inside them with room: the bounds are of the size of float32 roundings, not of the data
    res = GE.forward64(arrays, x.numpy(), ef.numpy(), w.numpy(), b.numpy(), beta, relu, 1e-7)
    tol = GE.forward_bounds(res, beta, EXP_ERR)
    assert float(tol["out"].max()) < 1e-3 and float(tol["lse"].max()) < 1e-2


# ------------------------------------------------------------------------------------------------ routing and refusals
def test_routing_and_refusals(monkeypatch):
    g = SG.small_graph(20, 30, 3)
    E = g.number_of_edges()
    x, ef, w, b, _ = _inputs(g, 4, 3, 0)
    with pytest.raises(ValueError, match="impl"):
        ops.u_add_e_softmax(g, x, ef, w, b, impl="triton")
    monkeypatch.setenv("BOT_SOFTMAX_AGG", "nothing")                  # read at call time
    with pytest.raises(ValueError, match="BOT_SOFTMAX_AGG"):
        ops.u_add_e_softmax(g, x, ef, w, b)
    monkeypatch.setenv("BOT_SOFTMAX_AGG", "tensor")
    assert ops.u_add_e_softmax(g, x, ef, w, b).shape == (20, 4)
    monkeypatch.delenv("BOT_SOFTMAX_AGG")
    from bot_amd import _C
    with pytest.raises(_C.BotKernelError, match="MI355X"):             # the kernel form has no CPU fallback
        ops.u_add_e_softmax(g, x, ef, w, b, impl="kernel")
    wide = torch.randn(E, 17)
    out = ops.u_add_e_softmax(g, x, wide, torch.randn(4, 17), b, impl="kernel")       # K > 16: the tensor form, whatever impl says
    assert out.shape == (20, 4)
    efg = ef.clone().requires_grad_()
    ops.u_add_e_softmax(g, x, efg, w, b, impl="kernel").sum().backward()              # ef asks for a gradient: the tensor form
    assert efg.grad is not None and bool(torch.isfinite(efg.grad).all())
    for bad, match in (((torch.randn(29, 4), ef, w, b), "source nodes"), ((torch.randn(30), ef, w, b), r"\[n_src, F\]"),
                       ((x, ef[:-1], w, b), "ef must be"), ((x, ef.reshape(-1), w, b), "ef must be"), ((x, ef[:, :0], w, b), "K >= 1"),
                       ((x, ef, w.t(), b), "weight must be"), ((x, ef, w, b[:3]), "bias must be"), ((x, ef.double(), w, b), "ef must be torch.float32"),
                       ((x, ef, w.double(), b), "weight must be torch.float32"), ((x, ef, w, b.double()), "bias must be torch.float32")):
        with pytest.raises(ValueError, match=match):
            ops.u_add_e_softmax(g, *bad)
    with pytest.raises(ValueError, match="beta"):
        ops.u_add_e_softmax(g, x, ef, w, b, torch.ones(2))
    with pytest.raises(ValueError, match="beta"):
        ops.u_add_e_softmax(g, x, ef, w, b, torch.ones(1, dtype=torch.float64))


def test_halo_plan_is_refused():
    g = SG.small_graph(20, 20, 3)
    g.halo = object()
    x, ef, w, b, _ = _inputs(g, 4, 3, 0)
    with pytest.raises(ValueError, match="halo"):
        ops.u_add_e_softmax(g, x, ef, w, b)
    with pytest.raises(ValueError, match="halo"):
        bnn.GENConv(4, 4, edge_dim=3)(g, x, ef)


# ------------------------------------------------------------------------------------------------ the layers
def test_state_dict_keys_with_and_without_edge_dim():
    plain = bnn.GENConv(6, 5, learn_beta=True)
    edge = bnn.GENConv(6, 5, learn_beta=True, edge_dim=8)
    assert set(edge.state_dict()) - set(plain.state_dict()) == {"lin_edge.weight", "lin_edge.bias"}
    assert set(plain.state_dict()) == {"beta", "mlp.0.weight", "mlp.0.bias"}
    assert edge.lin_edge.weight.shape == (6, 8) and "edge_dim=8" in repr(edge) and "edge_dim" not in repr(plain)
    stack = bnn.DeeperGCN(8, 5, 12, 3, edge_dim=4)
    assert all(f"convs.{i}.lin_edge.weight" in stack.state_dict() for i in range(3))
    assert stack.convs[0].lin_edge is not stack.convs[1].lin_edge
    assert not any("lin_edge" in k for k in bnn.DeeperGCN(8, 5, 12, 3).state_dict())
    with pytest.raises(ValueError, match="edge_dim"):
        bnn.GENConv(6, 5, edge_dim=0)
    sig = inspect.signature(bnn.DeeperGCN.forward)
    assert list(sig.parameters) == ["self", "graph", "feat", "edge_feats"] and sig.parameters["edge_feats"].default is None


@pytest.mark.parametrize("kw", [dict(), dict(learn_beta=True, msg_norm=True, learn_msg_scale=True, mlp_layers=2, beta=0.5)])
def test_genconv_edge_dim_against_fp64_restatement(backend, kw):
    g = SG.small_graph(65, 65, 7)
    conv = GE.check_conv(g, "cpu", 6, 5, 8, **kw)
    GE.check_conv(SG.small_graph(40, 130, 9), "cpu", 6, 5, 3, **kw)                    # a block-shaped graph
    E = g.number_of_edges()
    x = torch.randn(65, 6)
    with pytest.raises(ValueError, match="edge_feats"):
        conv(g, x)                                                                     # edge_dim set and no edge features
    with pytest.raises(ValueError, match="edge_feats"):
        conv(g, x, torch.randn(E, 6))                                                  # the encoded width is not the raw one
    with pytest.raises(ValueError, match="edge_feats"):
        conv(g, x, torch.randn(E - 1, 8))
    with pytest.raises(ValueError, match="edge_feats"):
        conv(g, x, torch.randn(E * 8))
    # without edge_dim the layer is what it was: encoded [E, in_feats] features, and today's message for another shape
    plain = bnn.GENConv(6, 5).eval()
    assert plain(g, x, torch.randn(E, 6)).shape == (65, 5)
    with pytest.raises(ValueError, match=r"edge_feats must be \[\d+, 6\] \(one row per edge, edge-id order\)"):
        plain(g, x, torch.randn(E, 8))


def test_deepergcn_edge_dim_against_fp64_restatement(backend):
    g = BC.parent_graph("cpu")
    gen = torch.Generator().manual_seed(2)
    ef = torch.rand(g.number_of_edges(), 8, generator=gen)
    torch.manual_seed(3)
    model = bnn.DeeperGCN(8, 5, 12, 3, dropout=0.5, learn_beta=True, edge_dim=8)
    GE.check_stack(model, g, g.ndata["feat"], ef, "cpu")
    # the three ways a Graph hands its edge features over give the same output
    model.eval()
    g.edata["feat"], g.edata["other"] = ef, ef
    with torch.no_grad():
        a, b, c = model(g, g.ndata["feat"], ef), model(g, g.ndata["feat"]), model(g, g.ndata["feat"], "other")
    assert torch.equal(a, b) and torch.equal(a, c)
    # blocks: a list of one tensor per block, or each block's rows of the parent's column
    seeds = torch.randperm(g.number_of_nodes(), generator=torch.Generator().manual_seed(3))[:150]
    blocks = BC.host_blocks(g, seeds, (4, 5, 6), 0)
    per_block = [b.edata["feat"] for b in blocks]
    assert all(e.shape == (b.number_of_edges(), 8) for e, b in zip(per_block, blocks))
    torch.manual_seed(4)
    GE.check_stack(bnn.DeeperGCN(8, 5, 12, 3, edge_dim=8), blocks, blocks[0].srcdata["feat"], per_block, "cpu")
    with torch.no_grad():
        assert torch.equal(model(blocks), model(blocks, None, per_block))
    with pytest.raises(ValueError, match="one per block"):
        model(blocks, None, per_block[:2])
    with pytest.raises(ValueError, match="one per block"):
        model(blocks, None, ef)
    del g.edata["feat"]
    with pytest.raises(ValueError, match="edata"):
        model(g, g.ndata["feat"])
    with pytest.raises(ValueError, match="edge_dim"):
        bnn.DeeperGCN(8, 5, 12, 3)(g, g.ndata["feat"], ef)


# ------------------------------------------------------------------------------------------------ the recipe
@pytest.mark.parametrize("learn_beta", [True, False])
def test_build_gen_edge_full_batch_step(backend, learn_beta):
    wl = workloads.build_gen_edge("proteins", "cpu", scale=0.002, learn_beta=learn_beta, drop=False)   # (the CPU emulation has no dropout stream)
    assert isinstance(wl.model, bnn.DeeperGCN) and len(wl.model.convs) == 3 and wl.model.convs[0]._out_feats == 256
    assert wl.model.edge_dim == 8 and wl.dataset.efeat.shape[1] == 8 and wl.dataset.n_classes == 112
    assert wl.dominant == ("spmm_softmax_edge", (256, 8, True, learn_beta)) and "edge_dim 8" in wl.describe
    loss, pred = wl.step()
    assert bool(torch.isfinite(loss)) and pred.shape == (wl.n_nodes, 112) and bool(torch.isfinite(pred).all())
    params = dict(wl.model.named_parameters())
    assert ("convs.0.beta" in params) == learn_beta and "convs.2.lin_edge.weight" in params
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params.values())
    assert all(float(params[f"convs.{i}.lin_edge.weight"].grad.abs().max()) > 0 for i in range(3))


def test_build_gen_edge_shapes_and_refusals():
    sig = inspect.signature(workloads.build_gen_edge)
    assert [p for p in sig.parameters][:2] == ["name", "device"]
    assert {k: v.default for k, v in sig.parameters.items() if v.kind is v.KEYWORD_ONLY} == dict(
        sampled=False, scale=1.0, seed=0, drop=True, learn_beta=True)
    for name in ("cora", "arxiv", "reddit", "products", "nothing"):
        with pytest.raises(ValueError, match="build_gen_edge"):
            workloads.build_gen_edge(name, "cpu")
    with pytest.raises(ValueError):
        workloads.build_gen("proteins", "cpu")              # build_gen is what it was


# ------------------------------------------------------------------------------------------------ the C ABI's checks, no GPU
def test_argument_validation_without_gpu():
    from bot_amd import _C
    lib = _C._lib
    buf = torch.zeros(512)
    p = buf.data_ptr()
    assert p % 16 == 0
    ok_f = dict(n=4, nnz=0, indices=None, items=p, long_rows=None, long_ptr=None, n_long=0, n_slots=0, x=p + 64, ldx=4, F=4, ef=None, K=8,
                eperm=None, wt=p + 512, bias=None, beta=p + 128, eps=0.0, out=p + 192, ldo=4, lse=p + 256, ldl=4, q=None, ldq=4, ws=None)
    ok_b = dict(n=4, nnz=0, indices=None, items=p, long_rows=None, long_ptr=None, n_long=0, x=p + 64, ldx=4, ef=None, K=8, eperm=None,
                wt=p + 512, bias=None, beta=p + 128, eps=0.0, dout=None, ldd=4, out=None, ldo=4, lse=None, ldl=4, F=4, dx=p + 192, lddx=4,
                partial=None, dweight=None, dw_ws=None, dw_rows=0)

    def fwd(**k):
        a = dict(ok_f, **k)
        return lib.bot_spmm_softmax_edge_f32(None, a["indices"], a["n"], a["nnz"], a["items"], 4, a["long_rows"], a["long_ptr"], a["n_long"],
                                             a["n_slots"], a["x"], a["ldx"], a["F"], a["ef"], a["K"], a["eperm"], a["wt"], a["bias"], a["beta"], 1,
                                             a["eps"], a["out"], a["ldo"], a["lse"], a["ldl"], a["q"], a["ldq"], a["ws"], None)

    def bwd(**k):
        a = dict(ok_b, **k)
        return lib.bot_spmm_softmax_edge_bwd_f32(None, a["indices"], a["n"], a["nnz"], a["items"], 4, a["long_rows"], a["long_ptr"], a["n_long"],
                                                 a["x"], a["ldx"], a["ef"], a["K"], a["eperm"], a["wt"], a["bias"], a["beta"], 1, a["eps"],
                                                 a["dout"], a["ldd"], a["out"], a["ldo"], a["lse"], a["ldl"], a["F"], a["dx"], a["lddx"],
                                                 a["partial"], a["dweight"], a["dw_ws"], a["dw_rows"], None)
    err = lib.bot_last_error
    for f in (fwd, bwd):
        assert f(n=0) == 0 and f(n=0, items=None, x=None) == 0                                  # an empty problem is a no-op
        assert f(F=0) == -2 and b"F=0" in err()
        assert f(n=-1) == -2 and f(nnz=-1) == -2 and f(n_long=-1) == -2 and b"negative" in err()
        assert f(n=2 ** 31) == -2 and f(nnz=2 ** 31 - 1) == -2 and b"int32" in err()
        assert f(eps=float("nan")) == -2 and f(eps=float("inf")) == -2 and b"eps" in err()
        assert f(K=0) == -2 and f(K=17) == -2 and f(K=-3) == -2 and b"K=" in err()
        assert f(wt=None) == -1 and b"ef/wt" in err()
        assert f(nnz=3, indices=p) == -1 and b"ef/wt" in err()                                  # edges without their features
        assert f(items=None) == -1 and f(x=None) == -1 and f(beta=None) == -1 and b"NULL" in err()
        assert f(nnz=3, ef=p + 1024) == -1 and b"indices" in err()                             # edges without their operands
        assert f(n_long=1, **({"n_slots": 2} if f is fwd else {})) == -1 and b"long rows" in err()
        assert f(ldx=3) == -2 and b"stride" in err()
        assert f(items=p + 4) == -3 and f(x=p + 66) == -3 and f(beta=p + 130) == -3 and f(wt=p + 514) == -3 and f(bias=p + 2) == -3 \
            and f(ef=p + 1026) == -3 and b"misaligned" in err()
    assert fwd(n_slots=-1) == -2
    assert fwd(out=None) == -1 and fwd(lse=None) == -1
    assert fwd(n_long=1, n_slots=0, long_rows=p, long_ptr=p, ws=p) == -2 and b"slots" in err()
    assert fwd(ldo=3) == -2 and fwd(ldl=3) == -2 and fwd(q=p + 320, ldq=3) == -2 and b"stride" in err()
    assert fwd(out=p + 64) == -2 and fwd(lse=p + 64) == -2 and fwd(q=p + 64) == -2 and fwd(lse=p + 192) == -2 and b"alias" in err()
    assert fwd(out=p + 194) == -3 and fwd(lse=p + 258) == -3 and fwd(q=p + 322) == -3 and fwd(eperm=p + 2, nnz=0) == -3
    assert bwd(dx=None) == 0                                                                    # neither dx nor dweight: nothing to do
    assert bwd(dweight=p + 768) == -1 and b"dw_workspace" in err()
    assert bwd(dw_rows=-1) == -2
    assert bwd(dx=p + 64) == -2 and b"alias" in err()
    assert bwd(lddx=3) == -2 and b"stride" in err()
    assert bwd(dx=p + 194) == -3 and bwd(dweight=p + 770, dw_ws=p + 1024) == -3 and bwd(dweight=p + 768, dw_ws=p + 1028) == -3
    # the binding's own checks: CPU tensors are refused before the library is entered
    g = SG.small_graph(20, 30, 3)
    with pytest.raises(_C.BotKernelError, match="MI355X"):
        _C.spmm_softmax_edge(g.csc, torch.zeros(30, 4), torch.zeros(g.number_of_edges(), 3), torch.zeros(4, 3), None, torch.ones(1))
    with pytest.raises(_C.BotKernelError, match="MI355X"):
        _C.spmm_softmax_edge_bwd(g.csr, torch.zeros(30, 4), torch.zeros(g.number_of_edges(), 3), torch.zeros(4, 3), None, torch.ones(1), True, 0.0,
                                 torch.zeros(20, 4), torch.zeros(20, 4), torch.zeros(20, 4))
    assert {"bot_spmm_softmax_edge_f32", "bot_spmm_softmax_edge_bwd_f32"} <= set(_C.EXPORTED) and _C.SOFTMAX_EDGE_MAX_K == 16
