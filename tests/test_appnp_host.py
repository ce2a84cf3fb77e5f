"""APPNP / GCNII without a GPU: the torch Philox mask against the numpy restatement, the tensor form of `ops.appnp_propagate` on CPU
float32 against the float64 restatement (tests/appnp_cases.py), the refusals, the C ABI's checks, and the four stacks."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bot_amd
from bot_amd import nn as bnn
from bot_amd import ops, smoothing, workloads
from tests import _oracle_backend
from tests import appnp_cases as AC
from tests import smooth_cases as SC


@pytest.fixture
def backend(monkeypatch):
    _oracle_backend.install(monkeypatch)
    monkeypatch.delenv("BOT_APPNP", raising=False)


# ------------------------------------------------------------------------------------------------ the mask
@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_appnp_keep_equals_the_numpy_mask_bit_for_bit(p):
    for step in (1, 7):
        for E in (1, 3, 4, 5, 4099):
            for seed in (0, 12345678901234567, -5, 2 ** 63 - 1):
                got = ops.appnp_keep(seed, step, E, p, "cpu")
                assert got.dtype == torch.bool and got.shape == (E,)
                assert np.array_equal(got.numpy(), AC.keep_mask(seed, step, E, p)), (p, step, E, seed)
    # steps and seeds give masks of their own
    assert not np.array_equal(AC.keep_mask(1, 1, 4099, p), AC.keep_mask(1, 2, 4099, p))
    assert not np.array_equal(AC.keep_mask(1, 1, 4099, p), AC.keep_mask(2, 1, 4099, p))


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_kept_share_at_one_half(seed):
    """50 000 positions at p = 0.5: the kept share within 5 sqrt(p (1 - p) / E) of 0.5 - the restatement alone first (the seeds were
    fixed after checking it), then the op's mask."""
    E, p = 50000, 0.5
    bound = 5.0 * (p * (1 - p) / E) ** 0.5
    assert abs(AC.keep_mask(seed, 1, E, p).mean() - 0.5) <= bound
    assert abs(ops.appnp_keep(seed, 1, E, p).float().mean().item() - 0.5) <= bound


# ------------------------------------------------------------------------------------------------ the tensor form on the CPU
def _frac(got, want, bound):
    """The largest |got - want| as a fraction of its bound (entries with a zero bound must agree exactly)."""
    err = (got.double() - want).abs()
    assert bool((err[bound == 0] == 0).all())
    return float((err / bound.clamp(min=1e-300)).max())


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("shared", [True, False])
@pytest.mark.parametrize("k,alpha", [(1, 0.5), (3, 0.1), (10, 0.1)])
def test_tensor_form_on_cpu_against_the_restatement(k, alpha, shared, p, weighted):
    src, dst, n = SC.graph("tiny")
    g = bot_amd.Graph(src, dst, n)
    gen = torch.Generator().manual_seed(1000 * k + 10 * int(shared) + int(weighted))
    ew = (0.5 + torch.rand(src.numel(), generator=gen)) if weighted else None
    x = torch.randn(n, 7, generator=gen).requires_grad_()
    h0 = None if shared else torch.randn(n, 7, generator=gen).requires_grad_()
    dout = torch.randn(n, 7, generator=gen)
    y = ops.appnp_propagate(g, x, k, alpha, h0=h0, edge_drop=p, seed=77, edge_weight=ew)
    y.backward(dout)
    ss, ds = smoothing._degree_scales(g, "DAD", smoothing._weights(g, ew))
    r = AC.propagate(src, dst, n, x.detach(), None if shared else h0.detach(), k, alpha, ss, ds, p=p, seed=77, ew=ew, dout=dout)
    assert _frac(y.detach(), r["h"], r["Eh"]) <= 1.0
    assert _frac(x.grad, r["dx"], r["Edx"]) <= 1.0
    if not shared:
        assert _frac(h0.grad, r["dh0"], r["Edh0"]) <= 1.0
    if p > 0:                                              # the same seed gives the same bytes, another seed another mask
        again = ops.appnp_propagate(g, x, k, alpha, h0=h0, edge_drop=p, seed=77, edge_weight=ew)
        other = ops.appnp_propagate(g, x, k, alpha, h0=h0, edge_drop=p, seed=78, edge_weight=ew)
        assert torch.equal(again, y) and not torch.equal(other, y)


def test_k_zero_returns_x_and_the_default_impl():
    src, dst, n = SC.graph("tiny")
    g = bot_amd.Graph(src, dst, n)
    x = torch.randn(n, 5)
    assert ops.appnp_propagate(g, x, 0, 0.1) is x
    from bot_amd import appnp
    assert appnp.default_impl(x) == "tensor" and appnp.default_impl(x, 0.5) == "tensor"
    with pytest.raises(ValueError, match="impl"):
        ops.appnp_propagate(g, x, 1, 0.1, impl="triton")


def test_refusals():
    src, dst, n = SC.graph("tiny")
    g = bot_amd.Graph(src, dst, n)
    x = torch.randn(n, 4)
    block = bot_amd.Graph(src[dst < 100], dst[dst < 100], n, num_dst_nodes=100)
    with pytest.raises(ValueError, match="square"):
        ops.appnp_propagate(block, x, 2, 0.1)
    halo = bot_amd.Graph(src, dst, n)
    halo.halo = object()                                   # a partition's graph carries a halo plan
    with pytest.raises(ValueError, match="square"):
        ops.appnp_propagate(halo, x, 2, 0.1)
    with pytest.raises(ValueError, match="edge_weight"):
        ops.appnp_propagate(g, x, 2, 0.1, edge_weight=torch.rand(src.numel(), requires_grad=True))
    for p in (1.0, 1.5, -0.1):
        with pytest.raises(ValueError, match="edge_drop"):
            ops.appnp_propagate(g, x, 2, 0.1, edge_drop=p)
    with pytest.raises(ValueError):
        ops.appnp_propagate(g, x[:-1], 2, 0.1)
    with pytest.raises(ValueError):
        ops.appnp_propagate(g, x, 2, 0.1, h0=torch.randn(n, 5))
    with pytest.raises(ValueError):
        ops.appnp_propagate(g, x, 2, 0.1, adj="DD")
    with pytest.raises(ValueError, match="block list"):
        bnn.APPNP(4, 3, 8, 2, F.relu)([block, block], x)
    with pytest.raises(ValueError, match="block list"):
        bnn.GCNII(4, 3, 8, 2, F.relu)([block, block], x)


def test_argument_validation_without_gpu():
    """bot_appnp_step_f32's checks run before any launch."""
    from bot_amd import _C
    lib = _C._lib
    buf = (ctypes.c_float * 64)()
    items = (ctypes.c_int32 * 16)()
    a = ctypes.addressof(buf)
    it = (ctypes.addressof(items) + 15) // 16 * 16 if ctypes.addressof(items) % 16 else ctypes.addressof(items)

    def call(n_rows=2, nnz=0, n_long=0, y=a, y0=None, out=a + 64, C=4, ld=4, acc_in=None, acc_out=None, partial=None, p=0.0, items_=it, indices=None):
        return lib.bot_appnp_step_f32(None, indices, n_rows, nnz, items_, 2, None, None, n_long, y, ld, y0, ld, out, ld, C, 0.9, 0.1, None, None, None,
                                      acc_in, ld, acc_out, ld, partial, None, None, p, 1, 1, None)
    assert call(n_rows=-1) == -2 and call(n_rows=2 ** 31) == -2 and call(nnz=2 ** 31) == -2
    assert call(C=0) == -2 and call(C=1025) == -2
    assert call(ld=3) == -2
    assert call(out=a) == -2 and b"aliases y" in lib.bot_last_error()
    assert call(acc_in=a + 128, acc_out=a) == -2
    for p in (1.0, -0.5, float("nan")):
        assert call(p=p) == -2
    assert call(y=None) == -1 and call(items_=None) == -1 and call(nnz=1) == -1
    assert call(acc_out=a + 128) == -1 and b"acc_out without acc_in" in lib.bot_last_error()
    assert call(n_long=1) == -1
    assert call(y=a + 2) == -3 and call(items_=it + 4) == -3
    assert call(n_rows=0) == 0                             # nothing launched


# ------------------------------------------------------------------------------------------------ layers and stacks
def _gcn2_case(project, seed, activation=None):
    src, dst, n = SC.graph("tiny")
    g = bot_amd.Graph(src, dst, n)
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    conv = bnn.GCN2Conv(6, layer=2, alpha=0.2, lambda_=0.5, project_initial_features=project, activation=activation)
    with torch.no_grad():
        conv.bias.copy_(torch.randn(6, generator=gen))
    feat, feat_0, dout = (torch.randn(n, 6, generator=gen) for _ in range(3))
    return g, (src, dst, n), conv, feat, feat_0, dout


def gcn2_grads(conv, graph, coo, feat, feat_0, dout, project, activation=None):
    """((out, grads by name) of the layer, the same of the float64 restatement)."""
    src, dst, n = coo
    f, f0 = feat.clone().requires_grad_(), feat_0.clone().requires_grad_()
    out = conv(graph, f, f0)
    out.backward(dout)
    got = {"feat": f.grad, "feat_0": f0.grad, **{k: v.grad for k, v in conv.named_parameters()}}
    p64 = {k: v.detach().cpu().double().requires_grad_() for k, v in conv.named_parameters()}
    d, d0 = feat.detach().cpu().double().requires_grad_(), feat_0.detach().cpu().double().requires_grad_()
    ref = AC.gcn2conv(src, dst, n, d, d0, p64["weight1"], p64.get("weight2"), p64["bias"], layer=2, alpha=0.2, lambda_=0.5,
                      project_initial_features=project, activation=activation)
    ref.backward(dout.cpu().double())
    want = {"feat": d.grad, "feat_0": d0.grad, **{k: v.grad for k, v in p64.items()}}
    return (out.detach(), got), (ref.detach(), want)


@pytest.mark.parametrize("project", [True, False])
def test_gcn2conv_against_the_restatement(backend, project):
    g, coo, conv, feat, feat_0, dout = _gcn2_case(project, 5)
    assert [k for k, _ in conv.named_parameters()] == (["weight1", "bias"] if project else ["weight1", "weight2", "bias"])
    (out, got), (ref, want) = gcn2_grads(conv, g, coo, feat, feat_0, dout, project)
    assert float((out.double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    for k in want:
        assert float((got[k].double() - want[k]).abs().max()) <= 1e-5 * float(want[k].abs().max()), k


def test_appnpconv_against_the_restatement(backend):
    src, dst, n = SC.graph("tiny")
    g = bot_amd.Graph(src, dst, n)
    conv = bnn.APPNPConv(4, 0.15, edge_drop=0.5)
    assert list(conv.parameters()) == []
    x = torch.randn(n, 5, generator=torch.Generator().manual_seed(0))
    conv.eval()
    ss, ds = smoothing._degree_scales(g, "DAD")
    r = AC.propagate(src, dst, n, x, None, 4, 0.15, ss, ds)
    out = conv(g, x)
    assert _frac(out, r["h"], r["Eh"]) <= 1.0 and torch.equal(conv(g, x), out)        # eval mode: no dropout, deterministic
    conv.train()
    torch.manual_seed(3)
    a = conv(g, x)
    torch.manual_seed(3)
    assert torch.equal(conv(g, x), a) and not torch.equal(a, out) and not torch.equal(conv(g, x), a)   # one seed per call, from torch's generator


def test_state_dict_keys_and_eval_determinism(backend):
    src, dst, n = SC.graph("tiny")
    g = bot_amd.Graph(src, dst, n)
    x = torch.randn(n, 9)
    m = bnn.APPNP(9, 4, 16, 3, F.relu, k=3)
    assert list(m.state_dict()) == ["lins.0.weight", "lins.0.bias", "lins.1.weight", "lins.1.bias", "lins.2.weight", "lins.2.bias"]
    mb = bnn.APPNP(9, 4, 16, 2, F.relu, norm="batch")
    assert [k for k in mb.state_dict() if "running" not in k and "tracked" not in k] == [
        "lins.0.weight", "lins.1.weight", "lins.1.bias", "norms.0.weight", "norms.0.bias"]
    m2 = bnn.GCNII(9, 4, 16, 3, F.relu)
    assert list(m2.state_dict()) == ["lins.0.weight", "lins.0.bias", "lins.1.weight", "lins.1.bias"] + [
        f"convs.{i}.{k}" for i in range(3) for k in ("weight1", "bias")]
    assert [abs(c.beta - np.log(0.5 / (i + 1) + 1)) < 1e-12 for i, c in enumerate(m2.convs)] == [True] * 3
    assert list(bnn.GCN2Conv(4, 1, project_initial_features=False, bias=False).state_dict()) == ["weight1", "weight2"]
    for model in (m, m2):
        model.eval()
        with torch.no_grad():
            a, b = model(g, x), model(g, x)
        assert a.shape == (n, 4) and torch.equal(a, b)
        model.train()
        out = model(g, x)
        out.sum().backward()
        assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in model.parameters())


@pytest.mark.parametrize("build,kind", [(workloads.build_appnp, bnn.APPNP), (workloads.build_gcn2, bnn.GCNII)])
def test_workloads_full_batch_step(backend, build, kind):
    wl = build("cora", "cpu", scale=0.25)
    assert isinstance(wl.model, kind) and wl.captured is False
    if kind is bnn.APPNP:
        assert len(wl.model.lins) == 2 and wl.model.lins[0].out_features == 64
        assert (wl.model.propagate._k, wl.model.propagate._alpha, wl.model.propagate.edge_drop) == (10, 0.1, 0.5)
    else:
        assert len(wl.model.convs) == 64 and wl.model.n_hidden == 64
    res = wl.step()
    assert bool(torch.isfinite(torch.as_tensor(res[0])).all())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in wl.model.parameters())
    with pytest.raises(ValueError):
        build("proteins", "cpu")
    import inspect
    sig = inspect.signature(build)
    assert {k: v.default for k, v in sig.parameters.items() if v.kind is v.KEYWORD_ONLY} == dict(scale=1.0, seed=0, drop=True)
