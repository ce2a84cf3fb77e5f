"""R-GCN without a GPU: `ops.rel_expand_sum` / `ops.rel_contract_sum` (the tensor form, which is what CPU tensors run),
`nn.RelGraphConv`, `nn.rel_norm` and `nn.RGCN` on CPU tensors against the float64 restatements (tests/rgcn_cases.py); the restatement's
gradients against torch.autograd.gradcheck; the derived bounds shown to catch three planted mistakes; impl selection, the error paths,
the layer's state_dict keys, `workloads.build_rgcn`, and the new symbols' argument checks.  tests/test_rgcn_gpu.py holds the kernels to
the same restatements."""
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
from tests import rgcn_cases as RC
from tests import sage_cases as SG

F64 = torch.float64


@pytest.fixture
def backend(monkeypatch):
    _oracle_backend.install(monkeypatch)
    monkeypatch.delenv("BOT_REL", raising=False)


def _blocks(g, fanouts, n_seeds=150, seed=0):
    seeds = torch.randperm(g.number_of_nodes(), generator=torch.Generator().manual_seed(seed + 3))[:n_seeds]
    return BC.host_blocks(g, seeds, fanouts, seed)


# ------------------------------------------------------------------------------------------------ the restatement itself
def test_restatement_gradients_against_gradcheck():
    """The gradients written from the formulas are the gradients of the sweeps: gradcheck of the float64 forward on a graph of 6 sources
    and 7 destinations, the last without in-edges, relation 3 of 4 without an edge."""
    src = torch.tensor([0, 1, 2, 2, 3, 5, 5, 4, 0, 1])
    dst = torch.tensor([1, 1, 0, 3, 3, 4, 2, 5, 0, 1])
    et = torch.tensor([0, 1, 2, 0, 0, 1, 2, 2, 1, 0])
    gen = torch.Generator().manual_seed(0)
    r = lambda *s: torch.randn(s, dtype=F64, generator=gen)
    c, coef, x, y, dZ, dout = r(10), r(4, 2).requires_grad_(), r(6, 3).requires_grad_(), r(6, 2, 3).requires_grad_(), r(7, 2, 3), r(7, 3)
    assert torch.autograd.gradcheck(lambda a, b: RC.expand64(src, dst, et, c, b, a, 7), (x, coef), eps=1e-6, atol=1e-6)
    assert torch.autograd.gradcheck(lambda a, b: RC.contract64(src, dst, et, c, b, a, 7), (y, coef), eps=1e-6, atol=1e-6)
    Z, out = RC.expand64(src, dst, et, c, coef, x, 7), RC.contract64(src, dst, et, c, coef, y, 7)
    assert bool((Z[6] == 0).all()) and bool((out[6] == 0).all())                        # a row without in-edges
    cd, xd, yd = coef.detach(), x.detach(), y.detach()
    for want, got, absg in ((torch.autograd.grad(Z, (x, coef), dZ), RC.expand_grads64(src, dst, et, c, cd, xd, dZ),
                             RC.expand_grads64(src, dst, et, c, cd, xd, dZ, absolute=True)),
                            (torch.autograd.grad(out, (y, coef), dout), RC.contract_grads64(src, dst, et, c, cd, yd, dout),
                             RC.contract_grads64(src, dst, et, c, cd, yd, dout, absolute=True))):
        for a, b, s in zip(got, want, absg):
            np.testing.assert_allclose(a.numpy(), b.numpy(), rtol=0, atol=1e-13)
            assert bool((a.abs() <= s + 1e-13).all())
        assert bool((got[1][3] == 0).all())                                                # the relation without an edge


@pytest.mark.parametrize("R,B", [(5, 2), (5, None), (40, 17)])
def test_bounds_catch_three_planted_mistakes(R, B):
    """The bounds are tight enough to mean something: a restatement that leaves out the last in-edge of the longest row, one with one
    edge's relation replaced by another, and one whose coefficients carry a relative error of 1e-5 exceed them somewhere in both
    sweeps' outputs; the restatement itself does not."""
    g = SG.small_graph(65, 90, 3)
    case = RC.normal_case(g, 5, R, B, 1)
    right, lim = RC.reference(g, case), RC.bounds(g, case)
    for mistake in ("drop", "relation", "coef"):
        wrong = RC.reference(g, case, mistake=mistake)
        for name in ("Z", "out"):
            assert bool(((wrong[name] - right[name]).abs() > lim[name]).any()), (mistake, name)
    for name in right:
        assert bool((lim[name] >= 0).all()) and lim[name].shape == right[name].shape
    # gamma(n + m + 2) at a row of 40 positions in chunks of 4: 52 roundings
    f = RC.expand_factor(torch.zeros(40, dtype=torch.int64), 1, 4)
    assert float(f[0]) == pytest.approx(52 * RC.U, rel=1e-5)
    assert float(RC.contract_factor(torch.zeros(40, dtype=torch.int64), 1, 64, 17)[0]) == pytest.approx((80 + 16 + 2) * RC.U, rel=1e-5)


# ------------------------------------------------------------------------------------------------ the ops on CPU tensors
@pytest.mark.parametrize("Fw", [1, 5, 64, 65])
@pytest.mark.parametrize("R,B", [(1, 1), (5, 2), (5, None), (40, 17)])
def test_tensor_form_against_fp64(backend, Fw, R, B):
    for i, g in enumerate((SG.small_graph(65, 65, 3), SG.small_graph(30, 90, 4))):          # isolated rows, parallel edges; a block
        got = RC.check_bounds(g, RC.normal_case(g, Fw, R, B, seed=Fw + i), "cpu", None)
        assert bool((got["Z"][g.in_degrees().cpu() == 0] == 0).all()) and bool((got["out"][g.in_degrees().cpu() == 0] == 0).all())
        RC.check_exact(g, RC.exact_case(g, Fw, R, B, seed=Fw + i), "cpu")
    assert "rel_expand_sum" in ops.__all__ and "rel_contract_sum" in ops.__all__ and ops.rel_default_impl in ops.REL_IMPLS


def test_one_hot_equals_basis_with_identity_coefficients(backend):
    """One-hot mode is basis mode with B = R and coef the identity, entry for entry in the exact regime."""
    g = SG.small_graph(30, 90, 4)
    case = RC.exact_case(g, 5, 5, None, seed=2)
    one = RC.run_ops(g, case, "cpu")
    two = RC.run_ops(g, dict(case, coef=torch.eye(5)), "cpu")
    for name in ("Z", "out", "dx", "dy"):
        assert torch.equal(one[name], two[name]), name
    no_norm = RC.run_ops(g, case, "cpu", norm=False)
    ones = RC.run_ops(g, dict(case, norm=torch.ones(g.number_of_edges())), "cpu")
    assert all(torch.equal(no_norm[k], ones[k]) for k in no_norm)


def test_edata_keys_and_integer_widths(backend):
    g = SG.small_graph(20, 30, 8)
    case = RC.normal_case(g, 4, 5, 2, 3)
    g.edata["etype"], g.edata["norm"] = case["et"].to(torch.int32), case["norm"].view(-1, 1)
    a = ops.rel_expand_sum(g, case["x"], "etype", 5, case["coef"], "norm")
    b = ops.rel_expand_sum(g, case["x"], case["et"], 5, case["coef"], case["norm"])
    assert torch.equal(a, b) and a.shape == (20, 2, 4)
    assert ops.rel_contract_sum(g, case["y"], "etype", 5, case["coef"]).shape == (20, 4)
    nm = case["norm"].clone().requires_grad_()                       # the norm is a constant: no gradient reaches it
    x = case["x"].clone().requires_grad_()
    ops.rel_expand_sum(g, x, case["et"], 5, case["coef"], nm).sum().backward()
    assert nm.grad is None and x.grad is not None


def test_cache_entries_leave_with_their_tensors(backend):
    """Relations and norms rewritten every epoch - as new tensors, or in place - do not pile up on a long-lived graph: the entries of
    tensors that are gone and of earlier versions leave when the next entry is made."""
    import gc
    g = SG.small_graph(20, 30, 8)
    E = g.number_of_edges()
    case = RC.normal_case(g, 4, 5, 2, 3)
    coef = case["coef"].clone().requires_grad_()
    sizes = []
    for epoch in range(5):                                           # new tensors (int64: an int32 copy, its position copies, a direction)
        et, nm = torch.randint(0, 5, (E,)), torch.rand(E)
        ops.rel_expand_sum(g, case["x"], et, 5, coef, nm).sum().backward()
        del et, nm
        gc.collect()
        sizes.append(len(g._bot_cache))
    assert len(set(sizes)) == 1, sizes
    et = torch.randint(0, 5, (E,), dtype=torch.int32)
    sizes = []
    for epoch in range(4):                                           # one tensor rewritten in place: a new version each time
        et[0] = epoch
        want = ops.rel_expand_sum(g, case["x"], et.clone(), 5, coef)
        assert torch.equal(ops.rel_expand_sum(g, case["x"], et, 5, coef), want)
        sizes.append(len(g._bot_cache))
    assert len(set(sizes)) == 1, sizes


def test_impl_selection_is_read_at_call_time(backend, monkeypatch):
    g = SG.small_graph(20, 30, 8)
    case = RC.normal_case(g, 4, 5, 2, 3)
    args = (g, case["x"], case["et"], 5, case["coef"], case["norm"])
    out = ops.rel_expand_sum(*args)
    monkeypatch.setenv("BOT_REL", "tensor")
    assert torch.equal(ops.rel_expand_sum(*args), out)
    monkeypatch.setenv("BOT_REL", "kernel")                      # the kernels have no CPU form: a missing kernel is an error
    with pytest.raises(_C.BotKernelError):
        ops.rel_expand_sum(*args)
    with pytest.raises(_C.BotKernelError):
        ops.rel_contract_sum(g, case["y"], case["et"], 5, case["coef"])
    assert torch.equal(ops.rel_expand_sum(*args, impl="tensor"), out)              # the argument wins over the variable
    monkeypatch.setenv("BOT_REL", "fast")
    with pytest.raises(ValueError, match="fast"):
        ops.rel_expand_sum(*args)


def test_error_paths(backend):
    g = SG.small_graph(20, 30, 8)
    E = g.number_of_edges()
    case = RC.normal_case(g, 4, 5, 2, 3)
    x, y, et, coef, nm = case["x"], case["y"], case["et"], case["coef"], case["norm"]
    for fn, bad, text in ((ops.rel_expand_sum, (x[:-1], et, 5, coef), "(29, 4)"), (ops.rel_expand_sum, (y, et, 5, coef), "(30, 2, 4)"),
                          (ops.rel_contract_sum, (x, et, 5, coef), "(30, 4)"), (ops.rel_contract_sum, (y, et, 5, None), "(30, 2, 4)"),
                          (ops.rel_expand_sum, (x, et[:-1], 5, coef), f"[{E}]"), (ops.rel_expand_sum, (x, et.float(), 5, coef), "float32"),
                          (ops.rel_expand_sum, (x, et, 5, coef[:4]), "(4, 2)"), (ops.rel_expand_sum, (x, et, 5, coef.double()), "float64"),
                          (ops.rel_expand_sum, (x, et, 5, coef, nm[:-1]), f"({E - 1},)"), (ops.rel_expand_sum, (x, et, 5, coef, nm.double()), "float64"),
                          (ops.rel_expand_sum, (x, et, 0, None), "num_rels"), (ops.rel_expand_sum, (x, "rel", 5, coef), "'rel'"),
                          (ops.rel_expand_sum, (x.long(), et, 5, None), "int64"), (ops.rel_expand_sum, (x, et, 3, None), "[0, num_rels = 3)"),
                          (ops.rel_contract_sum, (y, et - 1, 5, coef), "-1 .. ")):
        with pytest.raises(DGLError) as err:
            fn(g, *bad)
        assert text in str(err.value), (text, str(err.value))
    with pytest.raises(DGLError, match="float32"):
        ops.rel_expand_sum(g, x.double(), et, 5, coef.double(), impl="kernel")
    part = BC.parent_graph("cpu", n=200, e_raw=1500, seed=7)
    part.halo = object()                                             # a partition's block carries a halo plan
    pe = torch.zeros(part.number_of_edges(), dtype=torch.int64)
    with pytest.raises(ValueError, match="partition"):
        ops.rel_expand_sum(part, torch.randn(200, 4), pe, 1)
    with pytest.raises(ValueError, match="partition"):
        bnn.RelGraphConv(4, 4, 1)(part, torch.randn(200, 4), pe)
    with pytest.raises(NotImplementedError, match="bdd"):
        bnn.RelGraphConv(4, 4, 2, regularizer="bdd", num_bases=2)
    with pytest.raises(ValueError, match="regularizer"):
        bnn.RelGraphConv(4, 4, 2, regularizer="block")
    conv = bnn.RelGraphConv(4, 4, 5)
    conv.order = "sideways"
    with pytest.raises(ValueError, match="sideways"):
        conv(g, x, et)
    b = _loop_block()
    with pytest.raises(ValueError, match="destination"):
        bnn.RelGraphConv(4, 4, 1)(b, (torch.randn(50, 4), torch.randn(29, 4)), torch.zeros(b.number_of_edges(), dtype=torch.int64))
    with pytest.raises(ValueError, match="source nodes"):
        bnn.RelGraphConv(4, 4, 1)(b, torch.randn(30, 4), torch.zeros(b.number_of_edges(), dtype=torch.int64))
    with pytest.raises(DGLError, match="in_feat"):
        bnn.RelGraphConv(3, 4, 5)(g, x, et)


def _loop_block():
    from tests.gatv2_cases import loop_graph
    return loop_graph(30, 50, 11)


# ------------------------------------------------------------------------------------------------ the layer
@pytest.mark.parametrize("order", ["aggregate", "project"])
@pytest.mark.parametrize("num_bases", [2, None])
def test_relgraphconv_against_fp64_restatement(backend, order, num_bases):
    kw = dict(order=order, num_bases=num_bases)
    g = BC.parent_graph("cpu")                                       # square, with self-loops
    RC.check_conv(g, "cpu", 8, 5, 5, **kw)
    RC.check_conv(g, "cpu", 8, 6, 5, seed=1, bias=False, activation=F.elu, self_loop=False, with_norm=False, **kw)
    RC.check_conv(g, "cpu", 6, 8, 5, seed=2, layer_norm=True, activation=F.relu, **kw)
    b = _loop_block()
    RC.check_conv(b, "cpu", 6, 4, 5, seed=3, pair=True, **kw)       # a pair input
    RC.check_conv(b, "cpu", 6, 4, 5, seed=4, **kw)                  # one tensor: the first n_dst rows are the destinations
    blk = _blocks(g, (5,))[0]
    RC.check_conv(blk, "cpu", 8, 4, 5, seed=6, regularizer=None, **kw)        # a sampled block
    RC.check_conv(SG.small_graph(65, 65, 10), "cpu", 4, 3, 5, seed=7, **kw)   # zero in-degree rows


def test_order_rule_and_its_override(backend, monkeypatch):
    g = SG.small_graph(65, 65, 10)
    seen = []
    real_e, real_c = ops.rel_expand_sum, ops.rel_contract_sum
    monkeypatch.setattr(ops, "rel_expand_sum", lambda *a, **k: (seen.append("expand"), real_e(*a, **k))[1])
    monkeypatch.setattr(ops, "rel_contract_sum", lambda *a, **k: (seen.append("contract"), real_c(*a, **k))[1])
    _, up = RC.check_conv(g, "cpu", 4, 6, 5, seed=1, num_bases=2)                      # in <= out: aggregate first
    _, down = RC.check_conv(g, "cpu", 6, 4, 5, seed=1, num_bases=2)                    # in > out: project first
    _, same = RC.check_conv(g, "cpu", 4, 4, 5, seed=1, num_bases=2)
    assert seen == ["expand", "contract", "expand"]
    _, up_p = RC.check_conv(g, "cpu", 4, 6, 5, seed=1, num_bases=2, order="project")
    _, down_a = RC.check_conv(g, "cpu", 6, 4, 5, seed=1, num_bases=2, order="aggregate")
    assert seen[3:] == ["contract", "expand"]
    from tests.parity_cases import fwd_close
    fwd_close(up, up_p.numpy())
    fwd_close(down, down_a.numpy())


def test_one_relation_without_self_loop_is_graphconv(backend):
    g = BC.parent_graph("cpu")
    torch.manual_seed(0)
    ref = bnn.GraphConv(8, 5, norm="none", bias=True, allow_zero_in_degree=True)
    conv = bnn.RelGraphConv(8, 5, 1, self_loop=False)
    assert conv.w_comp is None and conv.weight.shape == (1, 8, 5)
    with torch.no_grad():
        conv.weight.copy_(ref.weight.unsqueeze(0))
        ref.bias.copy_(torch.randn(5))
        conv.h_bias.copy_(ref.bias)
    x = g.ndata["feat"]
    et = torch.zeros(g.number_of_edges(), dtype=torch.int64)
    from tests.parity_cases import fwd_close
    for order in ("aggregate", "project"):
        conv.order = order
        fwd_close(conv(g, x, et), ref(g, x).detach().numpy())


def test_parameters_and_state_dict_keys():
    conv = bnn.RelGraphConv(6, 4, 5, num_bases=2)
    assert {k: tuple(v.shape) for k, v in conv.state_dict().items()} == {"weight": (2, 6, 4), "w_comp": (5, 2), "h_bias": (4,), "loop_weight": (6, 4)}
    assert bool((conv.h_bias == 0).all())
    for kw in (dict(num_bases=5), dict(num_bases=None), dict(regularizer=None, num_bases=2), dict(num_bases=9), dict(num_bases=0)):
        conv = bnn.RelGraphConv(6, 4, 5, bias=False, self_loop=False, **kw)
        assert {k: tuple(v.shape) for k, v in conv.state_dict().items()} == {"weight": (5, 6, 4)} and conv.w_comp is None and conv.num_bases == 5
    conv = bnn.RelGraphConv(6, 4, 5, num_bases=3, layer_norm=True, low_mem=True)
    assert set(conv.state_dict()) == {"weight", "w_comp", "h_bias", "loop_weight", "layer_norm_weight.weight", "layer_norm_weight.bias"}
    assert isinstance(conv.layer_norm_weight, torch.nn.LayerNorm) and conv.layer_norm_weight.weight.shape == (4,)
    bound = np.sqrt(2.0) * np.sqrt(6.0 / (6 * 4 + 3 * 4))            # Xavier-uniform with the ReLU gain on [3, 6, 4]: fans 6 * 4 and 3 * 4
    assert float(conv.weight.detach().abs().max()) <= bound and float(conv.weight.detach().abs().max()) > 0.5 * bound
    sig = inspect.signature(bnn.RelGraphConv.__init__)
    assert list(sig.parameters)[1:] == ["in_feat", "out_feat", "num_rels", "regularizer", "num_bases", "bias", "activation", "self_loop",
                                        "low_mem", "dropout", "layer_norm"]
    assert sig.parameters["regularizer"].default == "basis" and sig.parameters["self_loop"].default is True
    assert all(n in bnn.__all__ for n in ("RelGraphConv", "RGCN", "rel_norm")) and bnn.__all__[-3:] == ["RelGraphConv", "RGCN", "rel_norm"]
    sig = inspect.signature(bnn.RGCN.__init__)
    assert list(sig.parameters)[1:] == ["in_feats", "n_classes", "n_hidden", "n_layers", "num_rels", "activation", "regularizer", "num_bases", "norm",
                                        "dropout", "input_drop", "self_loop"]


def test_rel_norm_against_a_numpy_count():
    g = SG.small_graph(65, 90, 3)
    src, dst, _, n_dst = RC.edge_lists(g)
    et = RC.relations(g, 5, 1)
    got = bnn.rel_norm(g, et, 5)
    count = np.zeros((n_dst, 5))
    np.add.at(count, (dst.numpy(), et.numpy()), 1)
    want = (1.0 / count[dst.numpy(), et.numpy()]).astype(np.float32).reshape(-1, 1)
    assert got.dtype == torch.float32 and np.array_equal(got.numpy(), want)
    assert bnn.rel_norm(g, et, 5) is got                             # once per graph
    g.edata["etype"] = et.to(torch.int32)
    assert torch.equal(bnn.rel_norm(g, "etype", 5), got)
    with pytest.raises(DGLError):
        bnn.rel_norm(g, et, 3)
    # with it every (destination, relation) group of in-edges sums to one
    tot = np.zeros((n_dst, 5))
    np.add.at(tot, (dst.numpy(), et.numpy()), got.numpy().ravel())
    assert np.allclose(tot[count > 0], 1.0)


# ------------------------------------------------------------------------------------------------ the stack, the recipe
def test_rgcn_stack_against_fp64_restatement(backend):
    g = BC.parent_graph("cpu")
    g.edata["etype"] = RC.relations(g, 5, 9)
    g.edata["norm"] = bnn.rel_norm(g, "etype", 5)
    torch.manual_seed(3)
    model = bnn.RGCN(8, 5, 6, 3, 5, F.relu, num_bases=2, norm="batch", dropout=0.5)
    assert len(model.norms) == 2 and model.norms[0].num_features == 6 and model.convs[0].h_bias is None and model.convs[2].h_bias is not None
    RC.check_stack(model, g, g.ndata["feat"], "cpu")
    blocks = _blocks(g, (4, 5, 6))
    model2 = bnn.RGCN(8, 5, 6, 3, 5, F.relu, regularizer=None)
    RC.check_stack(model2, blocks, blocks[0].srcdata["feat"], "cpu")
    out = model2.eval()(blocks, etypes=[b.edata["etype"] for b in blocks], norm=[b.edata["norm"] for b in blocks])       # given, not looked up
    assert torch.equal(out, model2(blocks))
    with pytest.raises(ValueError):
        model2(blocks[:2])
    with pytest.raises(ValueError, match="list"):
        model2(blocks, etypes=blocks[0].edata["etype"])
    with pytest.raises(TypeError):
        model(g)
    with pytest.raises(ValueError, match="norm"):
        bnn.RGCN(8, 5, 6, 3, 5, F.relu, norm="layer")
    bare = BC.parent_graph("cpu")
    with pytest.raises(DGLError, match="etype"):
        model(bare, bare.ndata["feat"])


def test_build_rgcn_full_batch_step(backend):
    wl = workloads.build_rgcn("cora", "cpu", scale=0.25)
    assert isinstance(wl.model, bnn.RGCN) and len(wl.model.convs) == 2 and len(wl.model.norms) == 0
    conv = wl.model.convs[0]
    assert conv.out_feat == 64 and conv.num_rels == 8 and conv.num_bases == 4 and conv.w_comp.shape == (8, 4) and "RGCN" in wl.describe
    et, nm = wl.graph.edata["etype"], wl.graph.edata["norm"]
    assert et.dtype == torch.int32 and int(et.min()) == 0 and int(et.max()) == 7 and nm.shape == (wl.graph.number_of_edges(), 1)
    loss, pred = wl.step()
    assert np.isfinite(float(loss.detach())) and bool(torch.isfinite(pred).all()) and pred.shape == (wl.n_nodes, wl.dataset.n_classes)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in wl.model.parameters())
    one_hot = workloads.build_rgcn("cora", "cpu", scale=0.25, regularizer=None)
    assert one_hot.model.convs[0].w_comp is None and one_hot.model.convs[0].weight.shape[0] == 8
    with pytest.raises(ValueError):
        workloads.build_rgcn("proteins", "cpu")
    sig = inspect.signature(workloads.build_rgcn)
    assert list(sig.parameters)[:2] == ["name", "device"]
    assert {k: v.default for k, v in sig.parameters.items() if v.kind is v.KEYWORD_ONLY} == dict(num_rels=8, regularizer="basis", num_bases=4,
                                                                                                 sampled=False, scale=1.0, seed=0, drop=True)


# ------------------------------------------------------------------------------------------------ the C ABI's checks, no GPU
@pytest.mark.parametrize("name", ["bot_spmm_rel_expand_f32", "bot_spmm_rel_contract_f32"])
def test_argument_validation_without_gpu(name):
    lib = _C._lib
    fn = getattr(lib, name)
    buf = torch.zeros(1024)
    p = buf.data_ptr()
    expand = "expand" in name
    call = lambda **k: fn(None, k.get("ind"), k.get("n", 4), k.get("nnz", 4), k.get("items"), 4, None, None, k.get("n_long", 0), k.get("n_slots", 0),
                          k.get("et"), k.get("norm"), k.get("coef"), k.get("R", 5), k.get("B", 2 if k.get("coef") else 0), k.get("x"), k.get("ldx", 8 if expand else 16),
                          k.get("F", 8), k.get("out"), k.get("ldo", 16 if expand else 8), k.get("ws"), None)
    assert call(F=0) == -2 and b"F=0" in lib.bot_last_error()
    assert call(R=0) == -2 and b"R=0" in lib.bot_last_error()
    assert call(coef=p, B=0) == -2 and b"B=0" in lib.bot_last_error()
    assert call(B=3) == -2 and b"one-hot" in lib.bot_last_error()                  # without coef: B is R or 0
    assert call(n=-1) == -2 and call(nnz=-1) == -2 and call(nnz=2 ** 31) == -2 and b"int32" in lib.bot_last_error()
    assert call(n=0) == 0                                                           # an empty problem is a no-op
    assert call(coef=p) == -1 and b"NULL" in lib.bot_last_error()
    ok = dict(ind=p, items=p, et=p + 64, coef=p + 128, x=p + 256, out=p + 2048)
    assert call(**{**ok, "et": None}) == -1 and b"etype" in lib.bot_last_error()
    assert call(**{**ok, "out": None}) == -1
    assert call(**ok, ldx=7) == -2 and b"stride" in lib.bot_last_error()
    assert call(**ok, ldo=7) == -2
    assert call(**{**ok, "out": p + 256}) == -2 and b"alias" in lib.bot_last_error()
    assert call(**{**ok, "x": p + 258}) == -3 and call(**ok, norm=p + 2) == -3 and call(**{**ok, "items": p + 8}) == -3
    assert call(**ok, n_long=1) == -1 and b"long rows" in lib.bot_last_error()
    assert call(**ok, F=2 ** 30, B=4, ldx=2 ** 40, ldo=2 ** 40) == -2 and b"B * F" in lib.bot_last_error()
    assert lib.bot_abi_version() == 19
