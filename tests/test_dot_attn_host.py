"""Dot-product attention without a GPU: `ops.dot_attention` (the tensor form, which is what CPU tensors run), `nn.DotGatConv`,
`nn.TransformerConv` and `nn.UniMP` on CPU tensors over the emulated backend against the float64 restatements (tests/dot_attn_cases.py);
the restatement's analytic gradients against torch.autograd.gradcheck; the exact regimes' conditions for the seeds the GPU tests use;
the layers' state_dict keys, every refusal, `workloads.build_unimp`, and the three entry points' argument checks.
tests/test_dot_attn_gpu.py holds the kernels to the same restatements."""
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bot_amd
from bot_amd import _C, ops, workloads
from bot_amd import nn as bnn
from bot_amd.errors import DGLError
from tests import _oracle_backend
from tests import block_cases as BC
from tests import dot_attn_cases as DC
from tests import gatv2_cases as GC
from tests import sage_cases as SG


@pytest.fixture
def backend(monkeypatch):
    _oracle_backend.install(monkeypatch)
    monkeypatch.delenv("BOT_DOT_ATTN", raising=False)


def _blocks(g, fanouts, n_seeds=150, seed=0):
    seeds = torch.randperm(g.number_of_nodes(), generator=torch.Generator().manual_seed(seed + 3))[:n_seeds]
    return BC.host_blocks(g, seeds, fanouts, seed)


# ------------------------------------------------------------------------------------------------ the restatement itself
def test_restatement_gradients_against_gradcheck():
    """The analytic gradients of the contract are the gradients of its forward: gradcheck of the float64 forward on a 6-node graph
    (with and without a keep mask), and `backward64` against autograd of it; lse against logsumexp."""
    src = torch.tensor([0, 1, 2, 2, 3, 5, 5, 4, 0, 1])
    dst = torch.tensor([1, 1, 0, 3, 3, 4, 2, 4, 0, 1])           # destination 5 has no in-edge
    gen = torch.Generator().manual_seed(0)
    H, D = 2, 3
    q, k, v = (torch.randn(6, H, D, dtype=torch.float64, generator=gen).requires_grad_() for _ in range(3))
    dout = torch.randn(6, H, D, dtype=torch.float64, generator=gen)
    for keep, c in ((None, 1.0), (DC.draw_keep(10, H, 0.4, 3), 1.0 / 0.6)):
        f = lambda a, b, cc: DC.attention64(src, dst, 6, a, b, cc, 0.7, keep, c)
        assert torch.autograd.gradcheck(f, (q, k, v), eps=1e-6, atol=1e-6)
        want = torch.autograd.grad(f(q, k, v), (q, k, v), dout)
        fwd = DC.forward64(src, dst, 6, q.detach(), k.detach(), v.detach(), 0.7, keep, c)
        bwd = DC.backward64(src, dst, 6, 6, q.detach(), k.detach(), v.detach(), 0.7, dout, fwd, keep, c)
        np.testing.assert_allclose(fwd["out"].numpy(), f(q, k, v).detach().numpy(), rtol=0, atol=1e-14)
        for name, w in zip(("dq", "dk", "dv"), want):
            np.testing.assert_allclose(bwd[name].numpy(), w.numpy(), rtol=0, atol=1e-13)
        s = (q.detach()[dst] * k.detach()[src]).sum(-1) * 0.7
        for r in range(5):
            np.testing.assert_allclose(fwd["lse"][r].numpy(), torch.logsumexp(s[dst == r], 0).numpy(), rtol=0, atol=1e-13)
        assert fwd["lse"][5].tolist() == [0.0, 0.0] and bool((fwd["out"][5] == 0).all())


def test_exact_regimes_hold_for_the_gpu_tests_seeds():
    """The conditions of the exact regimes are asserted while the inputs are built (tests/dot_attn_cases.onehot_inputs): every seed
    the GPU tests use passes here, without a GPU; both kinds of row - one maximal in-edge, and several parallel ones - occur."""
    from tests.test_dot_attn_gpu import EXACT_PAIRS, exact_seed, graph_specs
    singles = multis = 0
    for i, (name, make) in enumerate(graph_specs()):
        g = make()
        for H, D in EXACT_PAIRS:
            for shared in (False, True):
                case = DC.onehot_inputs(g, H, D, exact_seed(i, H, D), shared=shared)
                some = case["fwd"]["deg"] > 0
                singles += int(case["single"][some].sum())
                multis += int((~case["single"][some]).sum())
            DC.uniform_inputs(g, H, D, exact_seed(i, H, D))
    assert singles > 0 and multis > 0


def test_bounds_are_small_and_scale_with_the_lengths():
    g = SG.small_graph(65, 65, 3)
    src, dst = GC.positions(g)
    q, k, v, dout = (t.double() for t in DC.normal_inputs(65, 65, 3, 5, 0))
    fwd = DC.forward64(src, dst, 65, q, k, v, 5 ** -0.5)
    fb = DC.forward_bounds(fwd, 5)
    assert float(fb["out"].max()) < 1e-3 and float(fb["lse"].max()) < 1e-3
    assert float(fb["out"][3].max()) > float(fb["out"][0].max())            # row 3 has 40 in-edges
    bwd = DC.backward64(src, dst, 65, 65, q, k, v, 5 ** -0.5, dout, fwd)
    bb = DC.backward_bounds(src, dst, 65, 65, q, k, v, 5 ** -0.5, dout, fwd, bwd, fb, 5)
    assert all(float(bb[n].max()) < 1e-3 for n in ("dq", "dk", "dv"))


# ------------------------------------------------------------------------------------------------ the op on CPU tensors
@pytest.mark.parametrize("H,D", [(1, 1), (3, 5), (2, 64), (4, 65)])
def test_dot_attention_tensor_form_against_fp64(backend, H, D):
    for g in (SG.small_graph(65, 65, 3), SG.small_graph(30, 90, 4)):
        DC.check_op(g, "cpu", H, D, seed=H * D)
        DC.check_op(g, "cpu", H, D, seed=H * D + 1, shared=True)
        DC.check_op(g, "cpu", H, D, seed=H * D + 2, p=0.5)
    assert ops.dot_attn_last_impl == "tensor" and "dot_attention" in ops.__all__ and ops.dot_attn_default_impl in ops.DOT_ATTN_IMPLS
    assert bot_amd.dot_attention is ops.dot_attention


def test_dot_attention_autograd_wiring_against_finite_differences(backend):
    """A smoke check of the op's autograd wiring against finite differences, NOT a check of accuracy: the backend - the kernels, and
    their emulation here - is float32 only, so the step and tolerance are float32's (a few percent).  What holds the op's gradients
    to their values is `check_op`'s derived bounds against the float64 restatement, whose own gradients pass gradcheck in float64."""
    g = SG.small_graph(6, 9, 5)
    gen = torch.Generator().manual_seed(1)
    q = torch.randn(6, 2, 3, generator=gen).requires_grad_()
    k, v = (torch.randn(9, 2, 3, generator=gen).requires_grad_() for _ in range(2))
    kw = dict(eps=1e-2, atol=2e-2, rtol=2e-2, nondet_tol=0.0)
    assert torch.autograd.gradcheck(lambda a, b, c: ops.dot_attention(g, a, b, c, 0.6), (q, k, v), **kw)
    keep = DC.draw_keep(g.number_of_edges(), 2, 0.3, 2)
    assert torch.autograd.gradcheck(lambda a, b: ops.dot_attention(g, a, b, b, keep=keep, p=0.3), (q, k), **kw)


def test_uniform_and_onehot_regimes_on_the_tensor_form(backend):
    g = SG.small_graph(64, 130, 5)
    (q, k, v, dout), src, dst = DC.uniform_inputs(g, 3, 5, 7)
    out = ops.dot_attention(g, q, k, v)
    deg = GC.degree_of(dst, 64).view(-1, 1, 1)
    want = torch.zeros(64, 3, 5, dtype=torch.float64).index_add_(0, dst, v.double()[src]) / deg.clamp(min=1)
    np.testing.assert_allclose(out.double().numpy(), want.numpy(), rtol=0, atol=1e-5)
    case = DC.onehot_inputs(g, 3, 5, 7)
    out = ops.dot_attention(g, case["q"], case["k"], case["v"], case["scale"])
    np.testing.assert_allclose(out.double().numpy(), case["fwd"]["out"].numpy(), rtol=0, atol=1e-5)


def test_impl_selection_is_read_at_call_time(backend, monkeypatch):
    g = SG.small_graph(20, 30, 8)
    q, k, v = torch.randn(20, 2, 4), torch.randn(30, 2, 4), torch.randn(30, 2, 4)
    out = ops.dot_attention(g, q, k, v)
    monkeypatch.setenv("BOT_DOT_ATTN", "tensor")
    assert torch.equal(ops.dot_attention(g, q, k, v), out)
    monkeypatch.setenv("BOT_DOT_ATTN", "kernel")                  # the kernels have no CPU form: a missing kernel is an error
    with pytest.raises(_C.BotKernelError):
        ops.dot_attention(g, q, k, v)
    assert torch.equal(ops.dot_attention(g, q, k, v, impl="tensor"), out)         # the argument wins over the variable
    monkeypatch.setenv("BOT_DOT_ATTN", "fast")
    with pytest.raises(ValueError, match="fast"):
        ops.dot_attention(g, q, k, v)


def test_dot_attention_error_paths(backend):
    g = SG.small_graph(20, 30, 8)
    E = g.number_of_edges()
    q, k = torch.randn(20, 2, 4), torch.randn(30, 2, 4)
    assert ops.dot_attention(g, q, k, k).shape == (20, 2, 4)
    out, a = ops.dot_attention(g, q, k, k, return_attention=True)
    assert a.shape == (E, 2, 1)
    for bad, text in (((q[:-1], k, k), "(19, 2, 4)"), ((q, k[:, :1], k), "(30, 1, 4)"), ((q, k, q), "(20, 2, 4)"), ((q.view(20, 8), k, k), "(20, 8)")):
        with pytest.raises(ValueError) as err:
            ops.dot_attention(g, *bad)
        assert text in str(err.value)
    with pytest.raises(ValueError, match="keep"):
        ops.dot_attention(g, q, k, k, keep=torch.ones(E, 2), p=0.5)
    with pytest.raises(ValueError, match="p must"):
        ops.dot_attention(g, q, k, k, p=1.0)
    part = BC.parent_graph("cpu", n=200, e_raw=1500, seed=7)
    part.halo = object()                                             # a partition's block carries a halo plan
    with pytest.raises(ValueError, match="partition"):
        ops.dot_attention(part, torch.randn(200, 1, 4), torch.randn(200, 1, 4), torch.randn(200, 1, 4))
    for conv in (bnn.DotGatConv(4, 4, 1), bnn.TransformerConv(4, 4, 1)):
        with pytest.raises(ValueError, match="partition"):
            conv(part, torch.randn(200, 4))
    with pytest.raises(NotImplementedError, match="edge_dim"):
        bnn.TransformerConv(4, 4, 2, edge_dim=3)


def test_pack_keep_and_head_fit():
    keep = torch.zeros(3, 32, dtype=torch.bool)
    keep[0, 0] = keep[1, 31] = True
    keep[2] = True
    assert ops.pack_keep(keep).tolist() == [1, -2 ** 31, -1] and ops.pack_keep(keep).dtype == torch.int32
    t = lambda D: torch.zeros(4, 1, D)
    assert ops.dot_attn_head_fits(1536, t(1536)) and not ops.dot_attn_head_fits(1600, t(1600))
    assert ops.dot_attn_head_fits(384, t(384)[:, :, :383].contiguous()) is True and not ops.dot_attn_head_fits(385, t(385))


# ------------------------------------------------------------------------------------------------ the layers
def test_dotgatconv_against_fp64_restatement(backend):
    g = BC.parent_graph("cpu")                                       # square, with self-loops
    DC.check_layer(bnn.DotGatConv(8, 5, 3), DC.dotgat_conv64, g, "cpu", 8)
    b = GC.loop_graph(40, 90, 3)
    DC.check_layer(bnn.DotGatConv(6, 4, 2), DC.dotgat_conv64, b, "cpu", 6, seed=3, pair=True)
    DC.check_layer(bnn.DotGatConv(6, 4, 2), DC.dotgat_conv64, b, "cpu", 6, seed=4)       # one tensor: the first n_dst rows are the destinations
    blk = _blocks(g, (5,))[0]
    DC.check_layer(bnn.DotGatConv(8, 4, 2, allow_zero_in_degree=True), DC.dotgat_conv64, blk, "cpu", 8, seed=6)


@pytest.mark.parametrize("concat", [False, True])
@pytest.mark.parametrize("beta", [False, True])
@pytest.mark.parametrize("root_weight", [False, True])
def test_transformerconv_against_fp64_restatement(backend, concat, beta, root_weight):
    kw = dict(concat=concat, beta=beta, root_weight=root_weight)
    g = BC.parent_graph("cpu")
    torch.manual_seed(0)
    DC.check_layer(DC.seeded(bnn.TransformerConv(8, 5, 3, **kw), 0), DC.transformer_conv64, g, "cpu", 8)
    b = GC.loop_graph(40, 90, 3)
    DC.check_layer(DC.seeded(bnn.TransformerConv(6, 4, 2, bias=False, **kw), 1), DC.transformer_conv64, b, "cpu", 6, seed=3, pair=True)
    blk = _blocks(g, (5,))[0]
    DC.check_layer(DC.seeded(bnn.TransformerConv(8, 4, 1, allow_zero_in_degree=True, **kw), 2), DC.transformer_conv64, blk, "cpu", 8, seed=6)


def test_transformerconv_attention_dropout_against_the_same_mask(backend, monkeypatch):
    g = BC.parent_graph("cpu")
    conv = DC.seeded(bnn.TransformerConv(8, 5, 3, dropout=0.4), 0).train()
    keep = DC.draw_keep(g.number_of_edges(), 3, 0.4, 5)
    with monkeypatch.context() as m:
        m.setattr(torch, "rand", lambda *a, **k: keep.float())                     # rand >= p  <=>  keep (values 0 or 1 around p = 0.4)
        DC.check_layer(conv, DC.transformer_conv64, g, "cpu", 8, keep=keep)
    torch.manual_seed(0)
    a = conv(g, g.ndata["feat"])
    assert not torch.equal(a, conv(g, g.ndata["feat"])) and torch.equal(conv.eval()(g, g.ndata["feat"]), conv(g, g.ndata["feat"]))


def test_state_dict_keys_and_surfaces():
    conv = bnn.DotGatConv(6, 4, 3)
    assert set(conv.state_dict()) == {"fc.weight"} and conv.fc.weight.shape == (12, 6)
    with pytest.raises(DGLError):
        bnn.DotGatConv((6, 9), 4, 3)
    assert list(inspect.signature(bnn.DotGatConv.__init__).parameters)[1:] == ["in_feats", "out_feats", "num_heads", "allow_zero_in_degree"]
    conv = bnn.TransformerConv(6, 4, 3, beta=True)
    names = {"lin_key", "lin_query", "lin_value", "lin_skip"}
    assert set(conv.state_dict()) == {f"{n}.{p}" for n in names for p in ("weight", "bias")} | {"lin_beta.weight"}
    assert conv.lin_skip.weight.shape == (12, 6) and conv.lin_beta.weight.shape == (1, 36)
    conv = bnn.TransformerConv((6, 9), 4, 3, concat=False, beta=True, bias=False)
    assert set(conv.state_dict()) == {f"{n}.weight" for n in names | {"lin_beta"}}
    assert conv.lin_query.weight.shape == (12, 9) and conv.lin_skip.weight.shape == (4, 9) and conv.lin_beta.weight.shape == (1, 12)
    conv = bnn.TransformerConv(6, 4, 3, beta=True, root_weight=False)
    assert set(conv.state_dict()) == {f"{n}.{p}" for n in names - {"lin_skip"} for p in ("weight", "bias")}
    assert list(inspect.signature(bnn.TransformerConv.__init__).parameters)[1:10] == [
        "in_channels", "out_channels", "heads", "concat", "beta", "dropout", "edge_dim", "bias", "root_weight"]
    assert list(inspect.signature(bnn.UniMP.__init__).parameters)[1:] == [
        "in_feats", "n_classes", "n_hidden", "n_layers", "n_heads", "activation", "norm", "dropout", "input_drop", "attn_drop", "beta"]
    for name in ("DotGatConv", "TransformerConv", "UniMP"):
        assert name in bnn.__all__


def test_zero_in_degree_and_row_counts(backend):
    g = SG.small_graph(65, 65, 10)                                   # every fifth node has no in-edges
    x = torch.randn(65, 4)
    for make in (lambda **k: bnn.DotGatConv(4, 4, 2, **k), lambda **k: bnn.TransformerConv(4, 4, 2, root_weight=False, **k)):
        with pytest.raises(DGLError, match="0-in-degree"):
            make()(g, x)
        out = make(allow_zero_in_degree=True)(g, x)
        assert bool((out[g.in_degrees() == 0] == 0).all()) and bool(torch.isfinite(out).all())
    b = GC.loop_graph(30, 50, 11)
    with pytest.raises(ValueError, match="destination"):
        bnn.TransformerConv((4, 4), 4, 2)(b, (torch.randn(50, 4), torch.randn(29, 4)))
    with pytest.raises(ValueError, match="source nodes"):
        bnn.DotGatConv(4, 4, 2)(b, torch.randn(30, 4))


# ------------------------------------------------------------------------------------------------ the stack, the recipe
def test_unimp_stack_against_fp64_restatement(backend):
    g = BC.parent_graph("cpu")
    torch.manual_seed(3)
    model = bnn.UniMP(8, 5, 6, 3, 2, F.relu, norm="batch", dropout=0.5, attn_drop=0.1)
    assert len(model.norms) == 2 and model.norms[0].num_features == 12 and model.convs[0].concat and not model.convs[2].concat
    assert model.convs[2].lin_skip.weight.shape == (5, 12) and model.convs[0].lin_beta is not None
    DC.check_stack(model, g, g.ndata["feat"], "cpu")
    blocks = _blocks(g, (4, 5, 6))
    model2 = bnn.UniMP(8, 5, 6, 3, 2, F.relu, beta=False)
    DC.check_stack(model2, blocks, blocks[0].srcdata["feat"], "cpu")
    with pytest.raises(ValueError, match="edge_weight"):
        model(g, g.ndata["feat"], edge_weight=torch.ones(g.number_of_edges()))
    with pytest.raises(ValueError):
        model2(blocks[:2])
    with pytest.raises(ValueError, match="norm"):
        bnn.UniMP(8, 5, 6, 3, 2, F.relu, norm="layer")


def test_build_unimp_full_batch_step(backend):
    wl = workloads.build_unimp("cora", "cpu", scale=0.25)
    C = wl.dataset.n_classes
    assert isinstance(wl.model, bnn.UniMP) and len(wl.model.convs) == 2 and len(wl.model.norms) == 0 and "UniMP" in wl.describe
    assert wl.model.convs[0].lin_key.in_features == wl.dataset.feat.shape[1] + C and wl.step_kw["use_labels"]
    loss, pred = wl.step()
    assert np.isfinite(float(loss.detach())) and bool(torch.isfinite(pred).all()) and pred.shape == (wl.n_nodes, C)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in wl.model.parameters())
    wl = workloads.build_unimp("cora", "cpu", scale=0.25, use_labels=False)
    assert wl.model.convs[0].lin_key.in_features == wl.dataset.feat.shape[1] and not wl.step_kw["use_labels"]
    with pytest.raises(ValueError):
        workloads.build_unimp("proteins", "cpu")
    assert workloads.UNIMP_DIMS == {"cora": (2, 8, 8), "arxiv": (3, 3, 250), "reddit": (3, 1, 256)}
    sig = inspect.signature(workloads.build_unimp)
    assert {k: v.default for k, v in sig.parameters.items() if v.kind is v.KEYWORD_ONLY} == dict(sampled=False, scale=1.0, seed=0, drop=True,
                                                                                                 use_labels=True)


# ------------------------------------------------------------------------------------------------ the C ABI's checks, no GPU
def test_argument_validation_without_gpu():
    lib = _C._lib
    buf = torch.zeros(512)
    p = buf.data_ptr()
    g = lambda k, n, d=None: k.get(n, d)
    fwd = lambda **k: lib.bot_dot_attn_f32(None, g(k, "ind"), g(k, "n", 4), g(k, "nnz", 4), g(k, "items"), 4, None, None, g(k, "n_long", 0), 0,
                                           g(k, "q"), g(k, "ldq", g(k, "ld", 8)), g(k, "k"), g(k, "ld", 8), g(k, "v"), g(k, "ld", 8), g(k, "H", 2),
                                           g(k, "D", 4), g(k, "scale", 0.5), g(k, "keep"), g(k, "p", 0.0), g(k, "out"), g(k, "ld", 8), g(k, "lse"),
                                           g(k, "ldl", 2), None, None)
    dst = lambda **k: lib.bot_dot_attn_bwd_dst_f32(None, g(k, "ind"), g(k, "n", 4), 4, g(k, "items"), 4, None, None, g(k, "n_long", 0), g(k, "q"), 8,
                                                   g(k, "k"), 8, g(k, "v"), 8, g(k, "H", 2), g(k, "D", 4), g(k, "scale", 0.5), None, 0.0, g(k, "dout"), 8,
                                                   g(k, "out"), 8, g(k, "lse"), 2, g(k, "pw"), g(k, "ds"), g(k, "dq"), g(k, "lddq", 8), None, None)
    src = lambda **k: lib.bot_dot_attn_bwd_src_f32(None, g(k, "ind"), g(k, "n", 4), 4, g(k, "items"), 4, None, None, g(k, "n_long", 0), 0, g(k, "pos"),
                                                   g(k, "q"), 8, g(k, "dout"), 8, g(k, "pw"), g(k, "ds"), g(k, "H", 2), g(k, "D", 4), g(k, "scale", 0.5),
                                                   g(k, "dk"), g(k, "lddk", 8), g(k, "dv"), 8, None, None)
    nan = float("nan")
    assert fwd(H=0) == -2 and b"H=0" in lib.bot_last_error()
    assert fwd(D=0) == -2 and fwd(n=-1) == -2 and fwd(scale=nan) == -2 and b"NaN" in lib.bot_last_error()
    assert fwd(p=1.0) == -2 and fwd(n=0) == 0                                # an empty problem is a no-op
    assert fwd() == -1 and b"NULL" in lib.bot_last_error()
    ok = dict(ind=p, items=p, q=p + 64, k=p + 128, v=p + 192, out=p + 256, lse=p + 320)
    assert fwd(**ok, ldq=7) == -2 and b"stride" in lib.bot_last_error()
    assert fwd(**ok, ldl=1) == -2
    assert fwd(**{**ok, "out": p + 128}) == -2 and b"alias" in lib.bot_last_error()
    assert fwd(**{**ok, "q": p + 2}) == -3                                   # off its 4-byte alignment
    assert fwd(**ok, n_long=1) == -1                                         # long rows without their arrays
    assert fwd(**ok, keep=p, H=33) == -2 and b"bit per head" in lib.bot_last_error()
    assert fwd(**ok, H=1, D=1600, ld=1600) == -2 and b"does not fit" in lib.bot_last_error()      # a head wider than one tile: before any launch
    okb = dict(ok, dout=p + 384, pw=p + 448, ds=p + 512)
    assert dst(H=0) == -2 and dst(D=0) == -2 and dst(n=-1) == -2 and dst(scale=nan) == -2 and dst(n=0) == 0
    assert dst() == -1 and dst(**{**okb, "pw": None}) == -1 and b"NULL" in lib.bot_last_error()
    assert dst(**okb, dq=p + 576, lddq=7) == -2 and dst(**okb, dq=p + 128) == -2 and b"alias" in lib.bot_last_error()
    assert dst(**okb, dq=p + 576, n_long=1) == -1
    assert dst(**{**okb, "ds": p + 448}) == -2
    oks = dict(ind=p, items=p, pos=p, q=p + 64, dout=p + 384, pw=p + 448, ds=p + 512)
    assert src(H=0) == -2 and src(n=-1) == -2 and src(scale=nan) == -2 and src(n=0) == 0 and src() == 0      # neither gradient asked for
    assert src(dk=p + 576) == -1 and b"NULL" in lib.bot_last_error()
    assert src(**oks, dk=p + 576, lddk=7) == -2 and src(**oks, dk=p + 64) == -2 and b"alias" in lib.bot_last_error()
    assert src(**oks, dv=p + 384) == -2 and src(**oks, dk=p + 576, dv=p + 576, lddk=12) == -2
    assert src(**oks, dk=p + 576, n_long=1) == -1
    assert lib.bot_abi_version() == 19
