"""Dot-product attention with edge features without a GPU: the float64 restatements of tests/dot_attn_edge_cases.py against autograd and
gradcheck, the linearity identity the kernel form rests on, the bounds' non-vacuity (four wrong restatements), `ops.dot_attention_edge`
(the tensor form, which is what CPU tensors run), `nn.EdgeTransformerConv` and `nn.EdgeUniMP` on CPU tensors over the emulated backend,
state_dict keys, every argument check and refusal, `workloads.build_unimp_edge`, and the two entry points' argument checks.
tests/test_dot_attn_edge_gpu.py holds the kernels to the same restatements."""
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bot_amd
from bot_amd import _C, ops, workloads
from bot_amd import nn as bnn
from tests import _oracle_backend
from tests import block_cases as BC
from tests import dot_attn_cases as DC
from tests import dot_attn_edge_cases as EC
from tests import sage_cases as SG

F64 = torch.float64


@pytest.fixture
def backend(monkeypatch):
    _oracle_backend.install(monkeypatch)
    monkeypatch.delenv("BOT_DOT_ATTN", raising=False)


def _tiny():
    src = torch.tensor([0, 1, 2, 2, 3, 5, 5, 4, 0, 1, 1])
    dst = torch.tensor([1, 1, 0, 3, 3, 4, 2, 4, 0, 1, 1])           # destination 5 has no in-edge; 1 -> 1 is a parallel pair
    return src, dst


# ------------------------------------------------------------------------------------------------ the restatements themselves
def test_restatement_gradients_against_gradcheck_and_autograd():
    src, dst = _tiny()
    gen = torch.Generator().manual_seed(0)
    H, D, K = 2, 3, 2
    q, k, v = (torch.randn(6, H, D, dtype=F64, generator=gen).requires_grad_() for _ in range(3))
    ef = torch.randn(src.numel(), K, dtype=F64, generator=gen).requires_grad_()
    W = torch.randn(H * D, K, dtype=F64, generator=gen).requires_grad_()
    dout = torch.randn(6, H, D, dtype=F64, generator=gen)
    for keep, c in ((None, 1.0), (DC.draw_keep(src.numel(), H, 0.4, 3), 1.0 / 0.6)):
        f = lambda a, b, cc, w, e: EC.attention64(src, dst, 6, a, b, cc, e, w, 0.7, keep, c)
        assert torch.autograd.gradcheck(f, (q, k, v, W, ef), eps=1e-6, atol=1e-6)
        want = torch.autograd.grad(f(q, k, v, W, ef), (q, k, v, W, ef), dout)
        ref = EC.op_backward64(src, dst, 6, 6, q.detach(), k.detach(), v.detach(), ef.detach(), W.detach(), 0.7, dout, keep, c)
        np.testing.assert_allclose(ref["out"].numpy(), f(q, k, v, W, ef).detach().numpy(), rtol=0, atol=1e-14)
        for name, w in zip(("dq", "dk", "dv", "dW", "def_"), want):
            np.testing.assert_allclose(ref[name].numpy(), w.numpy(), rtol=0, atol=1e-13)
        # the kernel-level restatement: qe and daef as free operands
        qe = torch.randn(6, H, K, dtype=F64, generator=gen).requires_grad_()
        daef = torch.randn(6, H, K, dtype=F64, generator=gen)

        efc = ef.detach()

        def kernel_level(a, b, cc, e):
            s = ((a[dst] * b[src]).sum(-1) + (e[dst] * efc.unsqueeze(1)).sum(-1)) * 0.7
            ex = torch.exp(s)
            a_ = ex / torch.zeros(6, H, dtype=F64).index_add(0, dst, ex)[dst]
            w_ = a_ if keep is None else a_ * keep.double() * c
            return (torch.zeros(6, H, D, dtype=F64).index_add(0, dst, w_.unsqueeze(-1) * cc[src]),
                    torch.zeros(6, H, K, dtype=F64).index_add(0, dst, w_.unsqueeze(-1) * efc.unsqueeze(1)))
        o, ae = kernel_level(q, k, v, qe)
        want = torch.autograd.grad((o * dout).sum() + (ae * daef).sum(), (q, k, v, qe))
        fwd = EC.forward64(src, dst, 6, q.detach(), k.detach(), v.detach(), efc, qe.detach(), 0.7, keep, c)
        bwd = EC.backward64(src, dst, 6, 6, q.detach(), k.detach(), v.detach(), efc, qe.detach(), 0.7, dout, daef, fwd, keep, c)
        np.testing.assert_allclose(fwd["aef"].numpy(), ae.detach().numpy(), rtol=0, atol=1e-14)
        for name, w in zip(("dq", "dk", "dv", "dqe"), want):
            np.testing.assert_allclose(bwd[name].numpy(), w.numpy(), rtol=0, atol=1e-13)


def test_the_linearity_identity_the_kernel_form_rests_on():
    """sum p (v + W ef) = sum p v + W sum p ef, and <q, W ef> = <q W, ef>, in float64 to 1e-12."""
    g = SG.small_graph(30, 50, 3)
    src, dst = EC.positions(g)
    H, D, K = 3, 5, 4
    q, k, v, _, ef, W, _, _ = (t.double() for t in EC.normal_inputs(50, 30, src.numel(), H, D, K, 1))
    keep = DC.draw_keep(src.numel(), H, 0.3, 2)
    pyg = EC.attention64(src, dst, 30, q, k, v, ef, W, 0.4, keep, 1 / 0.7)
    W3 = W.view(H, D, K)
    qe = torch.einsum("nhd,hdk->nhk", q, W3)
    fwd = EC.forward64(src, dst, 30, q, k, v, ef, qe, 0.4, keep, 1 / 0.7)
    split = fwd["out"] + torch.einsum("nhk,hdk->nhd", fwd["aef"], W3)
    assert float((pyg - split).abs().max()) <= 1e-12
    E3 = (ef @ W.t()).view(-1, H, D)
    assert float(((q[dst] * E3).sum(-1) - (qe[dst] * ef.unsqueeze(1)).sum(-1)).abs().max()) <= 1e-12


def test_bounds_are_not_vacuous():
    """Four wrong restatements each exceed the bound of every output they can move, on seeded inputs for which the correct float32
    evaluation (the tensor form on the emulated backend is not used here: float32 torch of PyG's formula) stays under every bound.  The
    edge term dropped from the VALUE leaves p, and with it dv = sum p dout, unchanged: dv is left out for that one."""
    g = SG.small_graph(40, 40, 6)                                    # a whole graph: edge ids are not positions
    src, dst = EC.positions(g)
    eid = EC.eid_of_positions(g)
    assert not torch.equal(eid, torch.arange(eid.numel()))
    H, D, K = 3, 5, 3
    q, k, v, dout, ef, W, _, _ = EC.normal_inputs(40, 40, src.numel(), H, D, K, 4)
    sc = D ** -0.5
    a64 = [t.double() for t in (q, k, v, ef[eid], W)]
    ref = EC.op_backward64(src, dst, 40, 40, *a64, sc, dout.double())
    lim = EC.op_bounds(src, dst, 40, 40, *a64, sc, dout.double(), ref)

    def run(fn, dtype):
        leaves = [t.to(dtype).clone().requires_grad_() for t in (q, k, v, W, ef)]
        out = fn(*leaves)
        out.backward(dout.to(dtype))
        res = dict(zip(("out", "dq", "dk", "dv", "dW", "def_"), [out.detach().double()] + [t.grad.double() for t in leaves]))
        res["def_"] = res["def_"][eid]                              # edge-id order -> the restatement's positions
        return res

    def fracs(res):
        return {n: float(((res[n] - ref[n]).abs() / lim[n].clamp(min=1e-300)).max()) for n in lim}
    right = lambda a, b, c, w, e: EC.attention64(src, dst, 40, a, b, c, e[eid], w, sc)
    ok = fracs(run(right, torch.float32))
    assert all(f <= 1.0 for f in ok.values()), ok
    H_, D_ = H, D

    def no_value(a, b, c, w, e):                                     # the edge term dropped from the value
        return _split(a, b, c, w, e[eid], value=False)

    def no_key(a, b, c, w, e):                                       # ... from the key
        return _split(a, b, c, w, e[eid], key=False)

    def _split(a, b, c, w, e, key=True, value=True):
        E3 = (e @ w.t()).view(-1, H_, D_)
        s = (a[dst] * (b[src] + (E3 if key else 0))).sum(-1) * sc
        ex = torch.exp(s - s.detach().max())
        al = ex / torch.zeros(40, H_, dtype=s.dtype).index_add(0, dst, ex)[dst]
        return torch.zeros(40, H_, D_, dtype=s.dtype).index_add(0, dst, al.unsqueeze(-1) * (c[src] + (E3 if value else 0)))
    wrong = {
        "ef in edge-id order": lambda a, b, c, w, e: EC.attention64(src, dst, 40, a, b, c, e, w, sc),
        "no edge term in the value": no_value,
        "no edge term in the key": no_key,
        "W viewed [D, H, K]": lambda a, b, c, w, e: EC.attention64(src, dst, 40, a, b, c, e[eid], w.view(D_, H_, K).transpose(0, 1).reshape(H_ * D_, K), sc),
    }
    for name, fn in wrong.items():
        fr = fracs(run(fn, torch.float64))
        names = [n for n in fr if not (name == "no edge term in the value" and n == "dv")]
        assert all(fr[n] > 1.0 for n in names), (name, fr)


# ------------------------------------------------------------------------------------------------ the op on CPU tensors
@pytest.mark.parametrize("H,D,K", [(3, 5, 3), (2, 8, 8), (1, 1, 3)])
def test_tensor_form_against_fp64(backend, H, D, K):
    for g in (SG.small_graph(65, 65, 3), SG.small_graph(30, 90, 4)):
        EC.check_op(g, "cpu", H, D, K, seed=H * D + K)
        EC.check_op(g, "cpu", H, D, K, seed=H * D + K + 1, p=0.5)
        EC.check_op(g, "cpu", H, D, K, seed=H * D + K + 2, p=0.5, ef_grad=True)       # d ef too: only this form has it
    assert ops.dot_attn_last_impl == "tensor" and "dot_attention_edge" in ops.__all__


def test_tensor_form_autograd_wiring_against_finite_differences(backend):
    """A smoke check of the wiring for q, k, v, weight AND ef, not of accuracy: the emulated backend is float32 only, so step and
    tolerance are float32's.  `check_op`'s derived bounds hold the values."""
    g = SG.small_graph(6, 9, 5)
    E = g.number_of_edges()
    gen = torch.Generator().manual_seed(1)
    q = torch.randn(6, 2, 3, generator=gen).requires_grad_()
    k, v = (torch.randn(9, 2, 3, generator=gen).requires_grad_() for _ in range(2))
    ef, W = torch.randn(E, 2, generator=gen).requires_grad_(), torch.randn(6, 2, generator=gen).requires_grad_()
    kw = dict(eps=1e-2, atol=2e-2, rtol=2e-2, nondet_tol=0.0)
    assert torch.autograd.gradcheck(lambda a, b, c, e, w: ops.dot_attention_edge(g, a, b, c, e, w, 0.6), (q, k, v, ef, W), **kw)
    keep = DC.draw_keep(E, 2, 0.3, 2)
    assert torch.autograd.gradcheck(lambda a, e, w: ops.dot_attention_edge(g, a, k.detach(), v.detach(), e, w, keep=keep, p=0.3), (q, ef, W), **kw)


def test_argument_checks_and_refusals(backend, monkeypatch):
    g = SG.small_graph(20, 30, 8)
    E = g.number_of_edges()
    q, k, v = torch.randn(20, 2, 4), torch.randn(30, 2, 4), torch.randn(30, 2, 4)
    ef, W = torch.randn(E, 3), torch.randn(8, 3)
    out, a = ops.dot_attention_edge(g, q, k, v, ef, W, return_attention=True)
    assert out.shape == (20, 2, 4) and a.shape == (E, 2, 1) and ops.dot_attn_last_impl == "tensor"
    bad = [dict(q=q[:19]), dict(k=k[:, :1]), dict(v=torch.randn(30, 2, 5)), dict(ef=ef[:-1]), dict(ef=ef.view(-1)), dict(ef=torch.randn(E, 0)),
           dict(W=torch.randn(8, 4)), dict(W=torch.randn(3, 8)), dict(ef=ef.double()), dict(W=W.double()), dict(k=k.double()), dict(p=1.0),
           dict(p=-0.1), dict(keep=torch.ones(E, 3, dtype=torch.bool)), dict(keep=torch.ones(E, 2)), dict(impl="fast")]
    for kw in bad:
        a_ = dict(q=q, k=k, v=v, ef=ef, W=W)
        a_.update({n: kw[n] for n in kw if n in a_})
        rest = {n: kw[n] for n in kw if n not in a_}
        with pytest.raises(ValueError):
            ops.dot_attention_edge(g, a_["q"], a_["k"], a_["v"], a_["ef"], a_["W"], **rest)
    with pytest.raises(_C.BotKernelError):                            # the kernels have no CPU form: a missing kernel is an error
        ops.dot_attention_edge(g, q, k, v, ef, W, impl="kernel")
    halo = SG.small_graph(20, 30, 8)
    halo.halo = object()
    with pytest.raises(ValueError, match="halo"):
        ops.dot_attention_edge(halo, q, k, v, ef, W)
    with pytest.raises(NotImplementedError, match="edge_dim"):      # the pinned refusal stays
        bnn.TransformerConv(4, 4, 2, edge_dim=3)
    with pytest.raises(ValueError, match="edge_dim"):
        bnn.EdgeTransformerConv(4, 4, 2)
    conv = bnn.EdgeTransformerConv(4, 4, 2, edge_dim=3, allow_zero_in_degree=True)
    for e in (None, ef[:-1], torch.randn(E, 4)):
        with pytest.raises(ValueError, match="edge_attr"):
            conv(g, torch.randn(30, 4), e)
    assert workloads.build_unimp_edge.__name__ in dir(workloads) and bot_amd.nn.EdgeUniMP is bnn.EdgeUniMP


def test_state_dict_keys_and_surfaces():
    conv = bnn.EdgeTransformerConv(6, 4, 3, beta=True, edge_dim=5)
    names = {"lin_key", "lin_query", "lin_value", "lin_skip"}
    assert set(conv.state_dict()) == {f"{n}.{p}" for n in names for p in ("weight", "bias")} | {"lin_beta.weight", "lin_edge.weight"}
    assert conv.lin_edge.weight.shape == (12, 5) and conv.lin_edge.bias is None and isinstance(conv, bnn.TransformerConv)
    assert list(inspect.signature(bnn.EdgeTransformerConv.__init__).parameters)[1:] == [
        "in_channels", "out_channels", "heads", "concat", "beta", "dropout", "edge_dim", "bias", "root_weight", "allow_zero_in_degree"]
    assert list(inspect.signature(bnn.EdgeTransformerConv.forward).parameters)[1:] == ["graph", "feat", "edge_attr", "get_attention"]
    plain = bnn.UniMP(8, 5, 6, 3, 2, F.relu, norm="batch")
    edge = bnn.EdgeUniMP(8, 5, 6, 3, 2, F.relu, norm="batch", edge_dim=4)
    assert all(type(c) is bnn.TransformerConv for c in plain.convs) and all(type(c) is bnn.EdgeTransformerConv for c in edge.convs)
    assert not any("lin_edge" in n for n in plain.state_dict())
    assert set(edge.state_dict()) == set(plain.state_dict()) | {f"convs.{i}.lin_edge.weight" for i in range(3)}
    assert edge.convs[2].lin_edge.weight.shape == (10, 4) and edge.convs[0].lin_edge.weight.shape == (12, 4)
    with pytest.raises(ValueError, match="edge_dim"):
        bnn.EdgeUniMP(8, 5, 6, 3, 2, F.relu)
    for name in ("EdgeTransformerConv", "EdgeUniMP"):
        assert name in bnn.__all__


# ------------------------------------------------------------------------------------------------ layer, stack, recipe
def _with_edata(g, K, seed):
    g.edata["feat"] = torch.randn(g.number_of_edges(), K, generator=torch.Generator().manual_seed(seed))
    return g


@pytest.mark.parametrize("concat,beta", [(True, False), (False, True)])
def test_layer_against_fp64_restatement(backend, concat, beta):
    g = SG.small_graph(40, 40, 9)
    ef = torch.randn(g.number_of_edges(), 3, generator=torch.Generator().manual_seed(1))
    conv = DC.seeded(bnn.EdgeTransformerConv(6, 4, 2, concat=concat, beta=beta, edge_dim=3, allow_zero_in_degree=True), 0)
    EC.check_layer(conv, g, "cpu", 6, ef)
    b = SG.small_graph(30, 50, 10)
    ef = torch.randn(b.number_of_edges(), 3, generator=torch.Generator().manual_seed(2))
    EC.check_layer(DC.seeded(bnn.EdgeTransformerConv(6, 4, 2, concat=concat, beta=beta, edge_dim=3, allow_zero_in_degree=True), 1), b, "cpu", 6, ef,
                pair=True)


def test_stack_against_fp64_restatement_and_edge_feats_rules(backend):
    g = _with_edata(BC.parent_graph("cpu"), 4, 0)
    torch.manual_seed(3)
    model = bnn.EdgeUniMP(8, 5, 6, 3, 2, F.relu, norm="batch", dropout=0.5, attn_drop=0.1, edge_dim=4)
    EC.check_stack(model, g, g.ndata["feat"], "cpu")                                    # None: edata["feat"]
    g.edata["other"] = torch.randn(g.number_of_edges(), 4, generator=torch.Generator().manual_seed(5))
    EC.check_stack(model, g, g.ndata["feat"], "cpu", edge_feats="other")                # an edata key
    EC.check_stack(model, g, g.ndata["feat"], "cpu", edge_feats=g.edata["other"] * 2)   # a tensor
    seeds = torch.randperm(g.number_of_nodes(), generator=torch.Generator().manual_seed(3))[:150]
    blocks = BC.host_blocks(g, seeds, (4, 5, 6), 0)
    for b in blocks:
        assert tuple(b.edata["feat"].shape) == (b.number_of_edges(), 4)
    EC.check_stack(model, blocks, blocks[0].srcdata["feat"], "cpu")                     # each block's rows
    EC.check_stack(model, blocks, blocks[0].srcdata["feat"], "cpu", edge_feats=[b.edata["feat"] + 1 for b in blocks])
    with pytest.raises(ValueError, match="one per block"):
        model(blocks, edge_feats=blocks[0].edata["feat"])
    with pytest.raises(ValueError, match="edata"):
        model(g, g.ndata["feat"], edge_feats="missing")
    with pytest.raises(ValueError, match="edge_weight"):
        model(g, g.ndata["feat"], edge_weight=torch.ones(g.number_of_edges()))
    plain = bnn.UniMP(8, 5, 6, 3, 2, F.relu)
    with pytest.raises(ValueError, match="edge_feats only with edge_dim"):
        plain(g, g.ndata["feat"], edge_feats=g.edata["feat"])
    assert plain(g, g.ndata["feat"]).shape == (g.number_of_nodes(), 5)


def test_build_unimp_edge_full_batch_step(backend):
    wl = workloads.build_unimp_edge("proteins", "cpu", scale=0.002, drop=False)       # (the CPU emulation has no dropout stream)
    m = wl.model
    assert isinstance(m, bnn.EdgeUniMP) and len(m.convs) == 3 and m.convs[0].heads == 4 and m.convs[0].out_channels == 64
    assert m.convs[0].lin_edge.weight.shape == (256, 8) and len(m.norms) == 2 and "edge_dim 8" in wl.describe
    loss, pred = wl.step()
    assert np.isfinite(float(loss.detach())) and bool(torch.isfinite(pred).all()) and pred.shape == (wl.n_nodes, wl.dataset.n_classes)
    for name, p in m.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    # (layer 0 reads the raw node features, sums of up to hundreds of edge features: its gate sigmoid(lin_beta(.)) is saturated at
    # initialisation and passes the skip term alone, so that layer's attention parameters hold exact zeros; the later layers sit behind BatchNorm)
    assert all(float(m.convs[i].lin_edge.weight.grad.abs().max()) > 0 for i in (1, 2))
    for name in ("cora", "arxiv", "reddit", "products"):
        with pytest.raises(ValueError, match="build_unimp_edge"):
            workloads.build_unimp_edge(name, "cpu")
    with pytest.raises(ValueError):
        workloads.build_unimp("proteins", "cpu")
    sig = inspect.signature(workloads.build_unimp_edge)
    assert {k: v.default for k, v in sig.parameters.items() if v.kind is v.KEYWORD_ONLY} == dict(sampled=False, scale=1.0, seed=0, drop=True)


# ------------------------------------------------------------------------------------------------ the C ABI's checks, no GPU
_OUT = [torch.zeros(2048) for _ in range(3)]              # out, lse, aef: outputs may not alias inputs


def _fwd_args(p, n=4, nnz=6, H=2, D=4, K=3, ldqe=None, ldef=None, keep=None, prob=0.0, scale=1.0):
    HD, HK = H * D, H * K
    po, pl, pa = (t.data_ptr() for t in _OUT)
    return [p, p, n, nnz, p, n, None, None, 0, 0, p, HD, p, HD, p, HD, p, HK if ldqe is None else ldqe, p, K if ldef is None else ldef, H, D, K,
            scale, keep, prob, po, HD, pl, H, pa, HK, None, None]


def test_entry_point_argument_validation_without_gpu():
    lib = _C._lib
    assert {"bot_dot_attn_edge_f32", "bot_dot_attn_edge_bwd_dst_f32"} <= set(_C.EXPORTED) and lib.bot_abi_version() == 19
    buf = torch.zeros(2048)
    p = buf.data_ptr()
    err = lambda: lib.bot_last_error().decode()
    assert lib.bot_dot_attn_edge_f32(*_fwd_args(p, K=17)) == -2 and "K=17" in err()
    assert lib.bot_dot_attn_edge_f32(*_fwd_args(p, K=0)) == -2
    assert lib.bot_dot_attn_edge_f32(*_fwd_args(p, H=1, D=1, K=3)) == -2 and "D >= K" in err()
    assert lib.bot_dot_attn_edge_f32(*_fwd_args(p, H=1, D=1600, K=3, n=1, nnz=1)) == -2 and "does not fit" in err()
    assert lib.bot_dot_attn_edge_f32(*_fwd_args(p, ldqe=5)) == -2 and "row strides" in err()
    assert lib.bot_dot_attn_edge_f32(*_fwd_args(p, ldef=2)) == -2
    assert lib.bot_dot_attn_edge_f32(*_fwd_args(p, prob=1.0)) == -2
    assert lib.bot_dot_attn_edge_f32(*_fwd_args(p, scale=float("nan"))) == -2
    assert lib.bot_dot_attn_edge_f32(*_fwd_args(p, H=33, keep=p)) == -2 and "keep" in err()
    assert lib.bot_dot_attn_edge_f32(*_fwd_args(p, n=0)) == 0                               # an empty problem: nothing launched
    a = _fwd_args(p)
    a[16] = None                                                                            # qe
    assert lib.bot_dot_attn_edge_f32(*a) == -1 and "NULL" in err()
    a = _fwd_args(p)
    a[26] = p                                                                               # out aliases an input
    assert lib.bot_dot_attn_edge_f32(*a) == -2 and "alias" in err()
    a = _fwd_args(p)
    a[16] = p + 2                                                                           # a misaligned qe
    assert lib.bot_dot_attn_edge_f32(*a) == -3

    def bwd_args(H=2, D=4, K=3, n=4, nnz=6, **kw):
        HD, HK = H * D, H * K
        b = dict(q=p, qe=p, daef=p, dq=None, dqe=None, lddqe=HK, pw=pw_buf.data_ptr(), ds=ds_buf.data_ptr())
        b.update(kw)
        return [p, p, n, nnz, p, n, None, None, 0, 0, b["q"], HD, p, HD, p, HD, b["qe"], HK, p, K, H, D, K, 1.0, None, 0.0, p, HD, p, HD, p, H, p, HK,
                b["daef"], HK, b["pw"], b["ds"], b["dq"], HD, b["dqe"], b["lddqe"], None, None]
    f = lib.bot_dot_attn_edge_bwd_dst_f32
    pw_buf, ds_buf = torch.zeros(64), torch.zeros(64)
    assert f(*bwd_args(K=17)) == -2 and f(*bwd_args(H=1, D=2, K=3)) == -2 and f(*bwd_args(n=0)) == 0
    assert f(*bwd_args(daef=None)) == -1 and "NULL" in err()
    assert f(*bwd_args(ds=pw_buf.data_ptr())) == -2 and "alias" in err()
    out_ptr = torch.zeros(64).data_ptr()
    assert f(*bwd_args(dqe=out_ptr, lddqe=5)) == -2 and "row strides" in err()
    assert f(*bwd_args(dq=out_ptr, dqe=out_ptr)) == -2 and "alias" in err()


def test_onehot_regime_conditions_hold_for_the_gpu_tests_seeds():
    """The conditions `dot_attn_edge_cases.onehot_inputs` asserts (exact logits, no tie between distinct sources, a parallel pair that
    only its edge features separate, exact sums) for every graph, case and seed tests/test_dot_attn_edge_gpu.py uses - checked here, on
    the CPU, so that a GPU failure there is the kernel's."""
    from tests.test_dot_attn_gpu import exact_seed, graph_specs
    graphs = [make() for _, make in graph_specs()]
    for H, D, K in ((3, 5, 3), (2, 64, 8), (8, 32, 16), (4, 65, 8), (3, 250, 8), (8, 250, 1), (1, 16, 16)):
        for i, g in enumerate(graphs):
            seed = exact_seed(i, H, D) + K
            for p in (0.0, 0.5):
                keep = DC.draw_keep(g.number_of_edges(), H, p, seed + 1) if p > 0 else None
                case = EC.onehot_inputs(g, H, D, K, seed, keep=keep, c=1.0 / (1.0 - p))
                assert int(case["split"].sum()) > 0


def test_position_order_cache_belongs_to_the_tensor_handed_in(backend):
    """`ops.edge_features_csc`: the same tensor hits (the cached object comes back), a changed tensor misses (its version moved), and
    another tensor at a RECYCLED address with the same shape misses too - an entry is keyed by address, version and shape, and an
    address is free again once its tensor is."""
    g = SG.small_graph(20, 30, 8)
    E = g.number_of_edges()
    eid = g.csc.eid.long()
    ef = torch.randn(E, 3)
    rows = ops.edge_features_csc(g, ef)
    assert torch.equal(rows, ef[eid]) and ops.edge_features_csc(g, ef) is rows
    ef.mul_(2.0)
    again = ops.edge_features_csc(g, ef)
    assert again is not rows and torch.equal(again, ef[eid])
    key = ("ef_csc", ef.data_ptr(), ef._version, tuple(ef.shape))
    other = ef.detach().clone()
    g._bot_cache[key] = (g._bot_cache[key][0], torch.zeros(E, 3))             # what a dead tensor at this address would have left
    assert ops.edge_features_csc(g, ef) is g._bot_cache[key][1]                # the very tensor: a hit
    alias = ef.view(E, 3)                                                      # another tensor object over the same address, version and shape
    assert alias.data_ptr() == ef.data_ptr() and alias is not ef
    assert torch.equal(ops.edge_features_csc(g, alias), other[eid])            # not this tensor's entry: recomputed


def test_tensor_form_says_where_it_has_no_gradient(backend, monkeypatch):
    """Beyond 2^24 positions `graph.take_rows` gathers in pieces, which carry no gradient: the tensor form refuses with a ValueError
    that says so (here with the op's copy of the piece size lowered), and still runs the forward."""
    g = SG.small_graph(20, 30, 8)
    E = g.number_of_edges()
    q, k, v = torch.randn(20, 2, 4), torch.randn(30, 2, 4), torch.randn(30, 2, 4)
    ef, W = torch.randn(E, 3), torch.randn(8, 3)
    want = ops.dot_attention_edge(g, q, k, v, ef, W)
    monkeypatch.setattr(ops, "_TAKE_CHUNK", E - 1)
    assert torch.equal(ops.dot_attention_edge(g, q, k, v, ef, W), want)
    with torch.no_grad():
        assert torch.equal(ops.dot_attention_edge(g, q.clone().requires_grad_(), k, v, ef, W), want)
    for i in range(5):
        args = [q, k, v, ef, W]
        args[i] = args[i].clone().requires_grad_()
        with pytest.raises(ValueError, match="no gradient on a graph"):
            ops.dot_attention_edge(g, *args)
