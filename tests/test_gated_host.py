"""Gated aggregation without a GPU: `ops.gated_sum` (the tensor form, which is what CPU tensors run), `nn.ResGatedGraphConv` and
`nn.ResGatedGCN` on CPU tensors against the float64 restatements (tests/gated_cases.py); the restatement's gradients against
torch.autograd.gradcheck; the derived bounds shown to catch two planted mistakes; impl selection, the error paths, the layer's
state_dict keys, `workloads.build_gated`, and the new symbols' argument checks.  tests/test_gated_gpu.py holds the kernels to the same
restatements."""
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bot_amd import _C, ops, workloads
from bot_amd import nn as bnn
from bot_amd.errors import DGLError
from tests import _oracle_backend
from tests import block_cases as BC
from tests import gated_cases as GC
from tests import sage_cases as SG


@pytest.fixture
def backend(monkeypatch):
    _oracle_backend.install(monkeypatch)
    monkeypatch.delenv("BOT_GATE", raising=False)


def _blocks(g, fanouts, n_seeds=150, seed=0):
    seeds = torch.randperm(g.number_of_nodes(), generator=torch.Generator().manual_seed(seed + 3))[:n_seeds]
    return BC.host_blocks(g, seeds, fanouts, seed)


# ------------------------------------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("normalize", [False, True])
def test_restatement_gradients_against_gradcheck(normalize):
    """The gradients written from the formulas are the gradients of the forward: gradcheck of the float64 forward on a graph of 6 sources
    and 7 destinations, the last without in-edges, and `backward64` with the (a, b) of `upstream64` against autograd of it."""
    src = torch.tensor([0, 1, 2, 2, 3, 5, 5, 4, 0, 1])
    dst = torch.tensor([1, 1, 0, 3, 3, 4, 2, 5, 0, 1])
    gen = torch.Generator().manual_seed(0)
    Fw, eps = 3, 1e-3
    k = torch.randn(7, Fw, dtype=torch.float64, generator=gen).requires_grad_()
    q, v = (torch.randn(6, Fw, dtype=torch.float64, generator=gen).requires_grad_() for _ in range(2))
    assert torch.autograd.gradcheck(lambda a, b, c: GC.gated64(src, dst, a, b, c, normalize, eps), (k, q, v), eps=1e-6, atol=1e-6)
    dout = torch.randn(7, Fw, dtype=torch.float64, generator=gen)
    out = GC.gated64(src, dst, k, q, v, normalize, eps)
    want = torch.autograd.grad(out, (k, q, v), dout)
    kd, qd, vd = k.detach(), q.detach(), v.detach()
    fwd = GC.forward64(src, dst, kd, qd, vd, normalize, eps)
    np.testing.assert_allclose(fwd["out"].numpy(), out.detach().numpy(), rtol=0, atol=1e-14)
    assert bool((fwd["out"][6] == 0).all()) and bool((fwd["den"][6] == 0).all())          # a row without in-edges
    a, b = GC.upstream64(dout, fwd["out"], fwd["den"], normalize, eps)
    got, absg = GC.backward64(src, dst, kd, qd, vd, a, b)
    for x, y, c in zip(got, want, absg):
        np.testing.assert_allclose(x.numpy(), y.numpy(), rtol=0, atol=1e-13)
        assert bool((x.abs() <= c + 1e-13).all())


def test_restatement_gate_has_no_cancellation_in_either_tail():
    s = torch.tensor([-700.0, -40.0, -1.0, 0.0, 1.0, 40.0, 700.0], dtype=torch.float64)
    g, gbar = GC.gate64(s)
    assert g[3] == 0.5 and gbar[3] == 0.5 and torch.equal(g, gbar.flip(0))
    assert float(gbar[5]) == pytest.approx(np.exp(-40.0), rel=1e-15) and float(g[1]) == pytest.approx(np.exp(-40.0), rel=1e-15)
    assert float(torch.sigmoid(torch.tensor(120.0, dtype=torch.float64))) == 1.0


def test_bounds_catch_a_dropped_edge_and_a_gate_error():
    """The bounds are tight enough to mean something: a restatement that leaves out the last in-edge of one row, or whose gates carry a
    relative error of 1e-5, exceeds them; the restatement itself (error 0) and one with a gate error of 2 U do not."""
    g = SG.small_graph(65, 90, 3)
    src, dst = GC.positions(g)
    k, q, v, a, b = (t.double() for t in GC.normal_inputs(90, 65, 5, 1))
    eps = 1e-6
    bnd = GC.bounds(src, dst, k, q, v, a, b, eps)
    right = GC.forward64(src, dst, k, q, v, True, eps)
    row = int(torch.argmax(GC.degree_of(dst, 65)))
    dropped = GC.forward64(src, dst, k, q, v, True, eps, drop_last_of=row)
    for wrong in (dropped, GC.forward64(src, dst, k, q, v, True, eps, gate_error=1e-5)):
        assert bool(((wrong["num"] - right["num"]).abs() > bnd["num"]).any())
        assert bool(((wrong["den"] - right["den"]).abs() > bnd["den"]).any())
    assert bool(((dropped["out"] - right["out"]).abs() > bnd["out"])[row].any())
    near = GC.forward64(src, dst, k, q, v, True, eps, gate_error=2 * GC.U)
    for name in ("num", "den", "out"):
        assert bool(((near[name] - right[name]).abs() <= bnd[name]).all())
    # the same for the gradients: a gate error of 1e-5 on g' moves ds by 1e-5 of its absolute sum at least somewhere
    _, (adk, adq, adv) = GC.backward64(src, dst, k, q, v, a, b)
    for size, name in ((adk, "dk"), (adq, "dq"), (adv, "dv")):
        assert bool((1e-5 * size > bnd[name]).any()) and bool((2 * GC.U * size <= bnd[name]).all())
    assert bool((GC.bounds(src, dst, k, q, v, a, b, complement="subtracted")["dk"] >= bnd["dk"]).all())


# ------------------------------------------------------------------------------------------------ the op on CPU tensors
@pytest.mark.parametrize("Fw", [1, 5, 64, 65])
@pytest.mark.parametrize("normalize", [False, True])
def test_gated_sum_tensor_form_against_fp64(backend, Fw, normalize):
    for g in (SG.small_graph(65, 65, 3), SG.small_graph(30, 90, 4)):          # isolated rows, parallel edges; a block
        (out, _, _, _), _ = GC.check_op(g, "cpu", Fw, seed=Fw, normalize=normalize)
        assert bool((out[g.in_degrees().cpu() == 0] == 0).all())                    # zero in-degree rows
    assert "gated_sum" in ops.__all__ and ops.gate_default_impl in ops.GATE_IMPLS


def test_gated_sum_zero_eps_keeps_empty_rows_at_zero(backend):
    g = SG.small_graph(20, 30, 8)
    k, q, v, _, _ = GC.normal_inputs(30, 20, 4, 2)
    out = ops.gated_sum(g, k, q, v, normalize=True, eps=0.0)
    assert bool(torch.isfinite(out).all()) and bool((out[g.in_degrees() == 0] == 0).all())


def test_impl_selection_is_read_at_call_time(backend, monkeypatch):
    g = SG.small_graph(20, 30, 8)
    k, q, v, _, _ = GC.normal_inputs(30, 20, 4, 2)
    out = ops.gated_sum(g, k, q, v)
    monkeypatch.setenv("BOT_GATE", "tensor")
    assert torch.equal(ops.gated_sum(g, k, q, v), out)
    monkeypatch.setenv("BOT_GATE", "kernel")                     # the kernels have no CPU form: a missing kernel is an error
    with pytest.raises(_C.BotKernelError):
        ops.gated_sum(g, k, q, v)
    assert torch.equal(ops.gated_sum(g, k, q, v, impl="tensor"), out)              # the argument wins over the variable
    monkeypatch.setenv("BOT_GATE", "fast")
    with pytest.raises(ValueError, match="fast"):
        ops.gated_sum(g, k, q, v)
    assert ops.gate_default_impl in ("kernel", "tensor")


def test_gated_sum_error_paths(backend):
    g = SG.small_graph(20, 30, 8)
    k, q, v, _, _ = GC.normal_inputs(30, 20, 4, 2)
    assert ops.gated_sum(g, k, q, v).shape == (20, 4)
    for bad, text in (((k[:-1], q, v), "(19, 4)"), ((k, q[:-1], v), "(29, 4)"), ((k, q, v[:, :3]), "(30, 3)"), ((q, q, v), "(30, 4)"),
                      ((k.view(20, 2, 2), q, v), "(20, 2, 2)"), ((k, q, v.double()), "float64")):
        with pytest.raises(DGLError) as err:
            ops.gated_sum(g, *bad)
        assert text in str(err.value)
    with pytest.raises(ValueError, match="eps"):
        ops.gated_sum(g, k, q, v, normalize=True, eps=-1.0)
    part = BC.parent_graph("cpu", n=200, e_raw=1500, seed=7)
    part.halo = object()                                             # a partition's block carries a halo plan
    with pytest.raises(ValueError, match="partition"):
        ops.gated_sum(part, torch.randn(200, 4), torch.randn(200, 4), torch.randn(200, 4))
    with pytest.raises(ValueError, match="partition"):
        bnn.ResGatedGraphConv(4, 4)(part, torch.randn(200, 4))


# ------------------------------------------------------------------------------------------------ the layer
@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("root_weight", [False, True])
def test_resgatedgraphconv_against_fp64_restatement(backend, normalize, root_weight):
    kw = dict(normalize=normalize, root_weight=root_weight)
    g = BC.parent_graph("cpu")                                       # square, with self-loops
    GC.check_conv(g, "cpu", 8, 5, **kw)
    GC.check_conv(g, "cpu", 8, 6, seed=1, bias=False, activation=F.elu, **kw)
    b = GC.loop_graph(40, 90, 3)
    GC.check_conv(b, "cpu", (6, 7), 4, seed=3, pair=True, **kw)      # a pair input
    GC.check_conv(b, "cpu", 6, 4, seed=4, **kw)                      # one tensor: the first n_dst rows are the destinations
    blk = _blocks(g, (5,))[0]
    GC.check_conv(blk, "cpu", 8, 4, seed=6, **kw)                    # a sampled block
    GC.check_conv(SG.small_graph(65, 65, 10), "cpu", 4, 3, seed=7, **kw)          # zero in-degree rows


def test_resgatedgraphconv_parameters_and_state_dict_keys():
    conv = bnn.ResGatedGraphConv(6, 4)
    assert set(conv.state_dict()) == {"lin_key.weight", "lin_key.bias", "lin_query.weight", "lin_query.bias", "lin_value.weight",
                                      "lin_value.bias", "lin_skip.weight", "bias"}
    assert conv.lin_key.weight.shape == (4, 6) and conv.bias.shape == (4,) and bool((conv.bias == 0).all())
    conv = bnn.ResGatedGraphConv((6, 9), 4, root_weight=False, bias=False)
    assert set(conv.state_dict()) == {"lin_key.weight", "lin_key.bias", "lin_query.weight", "lin_query.bias", "lin_value.weight", "lin_value.bias"}
    assert conv.lin_key.weight.shape == (4, 9) and conv.lin_query.weight.shape == (4, 6) and conv.lin_skip is None and conv.bias is None
    sig = inspect.signature(bnn.ResGatedGraphConv.__init__)
    assert list(sig.parameters)[1:] == ["in_feats", "out_feats", "normalize", "eps", "root_weight", "bias", "feat_drop", "activation",
                                        "allow_zero_in_degree"]
    assert sig.parameters["normalize"].default is False and sig.parameters["eps"].default == 1e-6 and sig.parameters["allow_zero_in_degree"].default is True
    assert "ResGatedGraphConv" in bnn.__all__ and "ResGatedGCN" in bnn.__all__


def test_resgatedgraphconv_zero_in_degree_and_row_counts(backend):
    g = SG.small_graph(65, 65, 10)                                   # every fifth node has no in-edges
    x = torch.randn(65, 4)
    conv = bnn.ResGatedGraphConv(4, 4, root_weight=False, bias=False)
    out = conv(g, x)
    assert bool((out[g.in_degrees() == 0] == 0).all()) and bool(torch.isfinite(out).all())
    conv.set_allow_zero_in_degree(False)
    with pytest.raises(DGLError, match="0-in-degree"):
        conv(g, x)
    b = GC.loop_graph(30, 50, 11)
    with pytest.raises(ValueError, match="destination"):
        bnn.ResGatedGraphConv((4, 4), 4)(b, (torch.randn(50, 4), torch.randn(29, 4)))
    with pytest.raises(ValueError, match="source nodes"):
        bnn.ResGatedGraphConv(4, 4)(b, torch.randn(30, 4))


# ------------------------------------------------------------------------------------------------ the stack, the recipe
def test_resgatedgcn_stack_against_fp64_restatement(backend):
    g = BC.parent_graph("cpu")
    torch.manual_seed(3)
    model = bnn.ResGatedGCN(8, 5, 6, 3, F.relu, norm="batch", dropout=0.5, normalize=True)
    assert len(model.norms) == 2 and model.norms[0].num_features == 6 and model.convs[0].bias is None and model.convs[2].bias is not None
    GC.check_stack(model, g, g.ndata["feat"], "cpu")
    blocks = _blocks(g, (4, 5, 6))
    model2 = bnn.ResGatedGCN(8, 5, 6, 3, F.relu)
    GC.check_stack(model2, blocks, blocks[0].srcdata["feat"], "cpu")
    with pytest.raises(ValueError, match="edge_weight"):
        model(g, g.ndata["feat"], edge_weight=torch.ones(g.number_of_edges()))
    with pytest.raises(ValueError):
        model2(blocks[:2])
    with pytest.raises(TypeError):
        model(g)
    with pytest.raises(ValueError, match="norm"):
        bnn.ResGatedGCN(8, 5, 6, 3, F.relu, norm="layer")


def test_build_gated_full_batch_step(backend):
    wl = workloads.build_gated("cora", "cpu", scale=0.25)
    assert isinstance(wl.model, bnn.ResGatedGCN) and len(wl.model.convs) == 2 and len(wl.model.norms) == 0
    assert wl.model.convs[0]._out_feats == 64 and wl.model.convs[0].normalize and "ResGatedGCN" in wl.describe
    loss, pred = wl.step()
    assert np.isfinite(float(loss.detach())) and bool(torch.isfinite(pred).all()) and pred.shape == (wl.n_nodes, wl.dataset.n_classes)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in wl.model.parameters())
    with pytest.raises(ValueError):
        workloads.build_gated("proteins", "cpu")
    assert workloads.GATED_DIMS["arxiv"] == (3, 256)
    sig = inspect.signature(workloads.build_gated)
    assert list(sig.parameters)[:2] == ["name", "device"]
    assert {k: v.default for k, v in sig.parameters.items() if v.kind is v.KEYWORD_ONLY} == dict(sampled=False, normalize=True, scale=1.0, seed=0,
                                                                                                 drop=True)


# ------------------------------------------------------------------------------------------------ the C ABI's checks, no GPU
def test_argument_validation_without_gpu():
    lib = _C._lib
    buf = torch.zeros(512)
    p = buf.data_ptr()
    fwd = lambda **k: lib.bot_spmm_gate_f32(None, k.get("ind"), k.get("n", 4), k.get("nnz", 4), k.get("items"), 4, None, None, k.get("n_long", 0), 0,
                                            k.get("k"), k.get("ldk", 8), k.get("q"), 8, k.get("v"), 8, k.get("F", 8), k.get("norm", 0),
                                            k.get("eps", 1e-6), k.get("out"), k.get("ldo", 8), k.get("den"), 8, None, None)
    dst = lambda **k: lib.bot_spmm_gate_bwd_dst_f32(None, k.get("ind"), k.get("n", 4), 4, k.get("items"), 4, None, None, k.get("n_long", 0),
                                                    k.get("k"), 8, k.get("q"), 8, k.get("v"), 8, k.get("a"), 8, k.get("b"), k.get("ldb", 8),
                                                    k.get("F", 8), k.get("dk"), k.get("lddk", 8), None, None)
    src = lambda **k: lib.bot_spmm_gate_bwd_src_f32(None, k.get("ind"), k.get("n", 4), 4, k.get("items"), 4, None, None, k.get("n_long", 0), 0,
                                                    k.get("k"), 8, k.get("q"), 8, k.get("v"), 8, k.get("a"), 8, k.get("b"), 8, k.get("F", 8),
                                                    k.get("dq"), k.get("lddq", 8), k.get("dv"), 8, None, None)
    assert fwd(F=0) == -2 and b"F=0" in lib.bot_last_error()
    assert fwd(n=-1) == -2 and fwd(eps=float("nan")) == -2 and fwd(eps=float("inf")) == -2 and fwd(eps=-1e-6) == -2 and b"eps" in lib.bot_last_error()
    assert fwd() == -1 and b"NULL" in lib.bot_last_error()
    assert fwd(n=0) == 0                                               # an empty problem is a no-op
    ok = dict(ind=p, items=p, k=p + 64, q=p + 128, v=p + 192, out=p + 256)
    assert fwd(**ok, norm=1) == -1 and b"den" in lib.bot_last_error()  # the normalised form stores den
    assert fwd(**ok, ldk=7) == -2 and b"stride" in lib.bot_last_error()
    assert fwd(**ok, ldo=7) == -2
    assert fwd(**{**ok, "out": p + 128}) == -2 and b"alias" in lib.bot_last_error()
    assert fwd(**ok, norm=1, den=p + 256) == -2 and b"alias" in lib.bot_last_error()
    assert fwd(**{**ok, "q": p + 130}) == -3                           # off its 4-byte alignment
    assert fwd(**ok, n_long=1) == -1
    okb = dict(ind=p, items=p, k=p + 64, q=p + 128, v=p + 192, a=p + 256)
    assert dst(F=0) == -2 and dst(n=-1) == -2 and dst(n=0) == 0 and dst() == -1
    assert dst(**okb) == -1 and b"NULL" in lib.bot_last_error()        # no dk
    assert dst(**okb, dk=p + 320, lddk=7) == -2 and dst(**okb, dk=p + 320, b=p + 384, ldb=7) == -2
    assert dst(**okb, dk=p + 256) == -2 and b"alias" in lib.bot_last_error()
    assert dst(**okb, dk=p + 320, n_long=1) == -1
    assert dst(**{**okb, "a": p + 258}, dk=p + 320) == -3
    assert src(F=0) == -2 and src(n=-1) == -2 and src(n=0) == 0 and src() == 0          # neither gradient asked for: nothing to do
    assert src(dq=p + 320) == -1 and b"NULL" in lib.bot_last_error()
    assert src(**okb, dq=p + 320, lddq=7) == -2 and src(**okb, dq=p + 128) == -2 and b"alias" in lib.bot_last_error()
    assert src(**okb, dq=p + 320, dv=p + 320) == -2
    assert src(**okb, dv=p + 320, n_long=1) == -1
    assert lib.bot_abi_version() == 19
