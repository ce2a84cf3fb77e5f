"""The gated aggregation with an edge stream without a GPU: the float64 restatement (tests/gated_edge_cases.py) held to autograd, the
tensor form of `ops.gated_edge_sum` on CPU tensors under the derived bounds, `nn.GatedGCNConv` and `nn.GatedGCN` on CPU tensors against
their float64 restatements, names and shapes of the parameters, the refusals, the stack's permutation cache, and a demonstration that
the bounds bite.  The kernels themselves: tests/test_gated_edge_gpu.py."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bot_amd
from bot_amd import nn as bnn
from bot_amd import ops, workloads
from bot_amd.errors import DGLError
from tests import gated_edge_cases as EC
from tests import sage_cases as SG

DEV = "cpu"


def _graph(n_dst=40, n_src=40, seed=3):
    return SG.small_graph(n_dst, n_src, seed)


def _big():
    """About 5 000 edges in rows of 1 .. 11 and one of 40, with isolated rows and parallel edges: a wrong position cannot hide."""
    return SG.small_graph(1200, 1500, 21)


# ------------------------------------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("normalize", [False, True])
def test_restatement_gradients_are_autograd_of_the_float64_forward(normalize):
    g = _graph(12, 17, 5)
    src, dst = EC.positions(g)
    k, q, v, c, dout, _, de = (t.double() for t in EC.normal_inputs(17, 12, src.numel(), 3, 1))
    leaves = [t.clone().requires_grad_() for t in (k, q, v, c)]
    assert torch.autograd.gradcheck(lambda *x: EC.gated_edge64(src, dst, *x, normalize=normalize), leaves, eps=1e-6, atol=1e-7)
    out, e = EC.gated_edge64(src, dst, *leaves, normalize=normalize)
    torch.autograd.backward([out, e], [dout, de])
    fwd = EC.forward64(src, dst, k, q, v, c, normalize)
    assert torch.allclose(fwd["out"], out.detach(), rtol=0, atol=1e-13) and torch.equal(fwd["e"], e.detach())
    a, b = EC.upstream64(dout, fwd["out"], fwd["den"], normalize, 1e-6)
    want = EC.backward64(src, dst, fwd["e"], v, a, b, de)
    for name, leaf in zip(("dk", "dq", "dv", "ds"), leaves):
        assert torch.allclose(want[name], leaf.grad, rtol=1e-11, atol=1e-12), name


def test_exact_reference_agrees_with_the_float64_formulas():
    g = _graph(30, 45, 9)
    src, dst = EC.positions(g)
    k, q, v, c, a, b, de, s = EC.exact_inputs(src, dst, 45, 30, 5, 4)
    assert torch.equal((k[dst] + q[src]) + c, s) and set(s.unique().tolist()) == set(EC.REGIME_S)     # float32 arithmetic, exact
    ref = EC.exact_reference(src, dst, 45, 30, s, v, a, b, de)
    fwd = EC.forward64(src, dst, k.double(), q.double(), v.double(), c.double(), False)
    bwd = EC.backward64(src, dst, fwd["e"], v.double(), a.double(), b.double(), de.double())
    assert torch.equal(fwd["e"], ref["e"])
    for name, x in (("num", fwd["num"]), ("den", fwd["den"]), ("ds", bwd["ds"]), ("dk", bwd["dk"]), ("dq", bwd["dq"]), ("dv", bwd["dv"])):
        assert torch.allclose(x, ref[name], rtol=0, atol=1e-30 + 1e-40), name      # float64 leaves exp(-128) = 2.6e-56 where float32 has 0


# ------------------------------------------------------------------------------------------------ the tensor form on CPU tensors
@pytest.mark.parametrize("Fw", [1, 5, 64])
@pytest.mark.parametrize("normalize", [False, True])
def test_tensor_form_against_fp64_under_derived_bounds(Fw, normalize):
    worst = {}
    EC.check_op(_big(), DEV, Fw, seed=Fw, normalize=normalize, worst=worst)
    EC.check_op(_graph(63, 200, 8), DEV, Fw, seed=Fw + 1, normalize=normalize, worst=worst, with_de=False)
    assert worst and all(v <= 1.0 for v in worst.values())


def test_eid_order_is_csc_order_permuted_and_want_edge():
    g = _graph(50, 70, 6)                         # edge ids in no particular order
    perm = g.csc.eid.long()
    assert not torch.equal(perm, torch.arange(perm.numel()))
    k, q, v, c, dout, _, de = EC.normal_inputs(70, 50, perm.numel(), 4, 2)
    res = {}
    for order in ("csc", "eid"):
        leaves = [t.clone().requires_grad_() for t in (k, q, v, c)]
        out, e = ops.gated_edge_sum(g, *leaves, order=order)
        torch.autograd.backward([out, e], [dout, de])
        res[order] = (out, e) + tuple(t.grad for t in leaves)
    # the same numbers with c, e, dc and the upstream de renamed: compare through the edge's own row
    leaves = [t.clone().requires_grad_() for t in (k, q, v)]
    c_eid = torch.empty_like(c).index_copy_(0, perm, c).requires_grad_()
    out, e = ops.gated_edge_sum(g, *leaves, c_eid, order="eid")
    torch.autograd.backward([out, e], [dout, torch.empty_like(de).index_copy_(0, perm, de)])
    want = res["csc"]
    assert torch.equal(out, want[0]) and torch.equal(e[perm], want[1]) and torch.equal(c_eid.grad[perm], want[5])
    assert all(torch.equal(a.grad, b) for a, b in zip(leaves, want[2:5]))
    out2, none = ops.gated_edge_sum(g, k, q, v, c, order="csc", want_edge=False)
    assert none is None and torch.equal(out2, want[0])
    plain, _ = ops.gated_edge_sum(g, k, q, v, c, normalize=False, order="csc")
    fwd = EC.forward64(*EC.positions(g), k.double(), q.double(), v.double(), c.double(), False)
    assert torch.allclose(plain.double(), fwd["num"], atol=1e-4)
    assert bool((want[0][torch.diff(g.csc.indptr) == 0] == 0).all())                  # isolated destinations: exactly 0


def test_impl_selection(monkeypatch):
    g = _graph()
    k, q, v, c = EC.normal_inputs(40, 40, g.number_of_edges(), 3, 1)[:4]
    assert ops.gate_edge_default_impl == "kernel"
    monkeypatch.setenv("BOT_GATE_EDGE", "nonsense")
    with pytest.raises(ValueError, match="BOT_GATE_EDGE"):
        ops.gated_edge_sum(g, k, q, v, c)
    assert ops.gated_edge_sum(g, k, q, v, c, impl="tensor")[0].shape == (40, 3)       # the argument wins over the variable
    monkeypatch.setenv("BOT_GATE_EDGE", "kernel")
    with pytest.raises(Exception, match="MI355X|CPU"):                                 # no quiet fall-back: the kernels take GPU tensors
        ops.gated_edge_sum(g, k, q, v, c)


def test_entry_points_check_their_arguments_before_any_launch():
    """What include/bot_gnn.h lists as checked before any launch, without a GPU: sizes, F, eps, NULL operands, strides, aliases,
    alignment; empty problems and absent outputs are no-ops."""
    from bot_amd import _C
    lib = _C._lib
    N = None
    x = torch.zeros(64, dtype=torch.float32)                                # a host buffer: only its address is looked at
    p, q = x.data_ptr(), x.data_ptr() + 16
    fwd = lambda **o: lib.bot_spmm_gate_edge_f32(N, o.get("indices", p), o.get("n", 4), o.get("nnz", 4), o.get("items", p), 4, N, N, 0, 0,
                                                 o.get("k", p), o.get("ldk", 4), p, 4, p, 4, o.get("c", p), 4, o.get("F", 4), o.get("norm", 0),
                                                 o.get("eps", 1e-6), o.get("out", q), 4, o.get("den", N), 4, o.get("e", N), o.get("lde", 4), 0, N, N)
    assert fwd(F=0) == -2 and b"F=0" in lib.bot_last_error()
    assert fwd(eps=float("nan")) == -2 and fwd(eps=-1.0) == -2 and fwd(n=-1) == -2
    assert fwd(n=0) == 0
    assert fwd(k=N) == -1 and fwd(c=N) == -1 and fwd(norm=1) == -1 and b"NULL" in lib.bot_last_error()
    assert fwd(ldk=3) == -2 and b"row strides" in lib.bot_last_error()
    assert fwd(out=p) == -2 and b"alias" in lib.bot_last_error()
    assert fwd(e=q) == -2                                                   # e aliasing out
    assert fwd(e=p, lde=8) == -2                                            # e may be c itself only with c's pitch
    assert fwd(c=p + 2) == -3 and b"misaligned" in lib.bot_last_error()
    bwd = lambda **o: lib.bot_spmm_gate_edge_bwd_f32(N, p, o.get("n", 4), 4, p, 4, N, N, 0, p, 4, o.get("e", p), 4, o.get("a", p), 4, N, 4,
                                                     o.get("de", N), o.get("ldde", 4), o.get("F", 4), o.get("ds", q), o.get("ldds", 4),
                                                     o.get("dk", N), 4, 0, N, N)
    assert bwd(F=0) == -2 and bwd(n=0) == 0 and bwd(ds=N, dk=N) == 0        # neither output: nothing to do
    assert bwd(a=N) == -1 and bwd(e=N) == -1
    assert bwd(ds=p) == -2 and b"alias" in lib.bot_last_error()
    assert bwd(de=q, ds=q, ldds=8) == -2                                    # ds may be de itself only with de's pitch
    src = lambda **o: lib.bot_spmm_gate_edge_bwd_src_f32(N, p, o.get("n", 4), 4, p, 4, N, N, 0, 0, o.get("pos", p), o.get("e", p), 4,
                                                         o.get("ds", p), 4, o.get("a", p), 4, o.get("F", 4), o.get("dq", q), 4, o.get("dv", N), 4, N, N)
    assert src(F=0) == -2 and src(n=0) == 0 and src(dq=N, dv=N) == 0
    assert src(ds=N) == -1 and src(pos=N) == -1 and src(dq=N, dv=q, e=N) == -1
    assert src(dq=p) == -2 and src(dq=q, dv=q) == -2


# ------------------------------------------------------------------------------------------------ layer and stack
def test_state_dict_keys_and_shapes():
    conv = bnn.GatedGCNConv(6, 3, 5)
    sd = conv.state_dict()
    want = {f"{n}.{w}" for n in "ABCDE" for w in ("weight", "bias")}
    want |= {f"{bn}.{w}" for bn in ("bn_node", "bn_edge") for w in ("weight", "bias", "running_mean", "running_var", "num_batches_tracked")}
    assert set(sd) == want
    assert all(sd[f"{n}.weight"].shape == (5, 6) and sd[f"{n}.bias"].shape == (5,) for n in "ABDE")
    assert sd["C.weight"].shape == (5, 3) and sd["bn_node.weight"].shape == (5,) and sd["bn_edge.running_var"].shape == (5,)
    assert not conv.residual and bnn.GatedGCNConv(5, 5, 5).residual and not bnn.GatedGCNConv(5, 5, 5, residual=False).residual
    assert "GatedGCNConv" in bnn.__all__ and "GatedGCN" in bnn.__all__
    model = bnn.GatedGCN(7, 3, 4, 6, 3)
    keys = set(model.state_dict())
    assert {"embedding_h.weight", "embedding_e.weight", "out.bias", "convs.2.E.bias", "convs.0.bn_edge.weight"} <= keys
    assert model.state_dict()["embedding_e.weight"].shape == (6, 3) and model.state_dict()["out.weight"].shape == (4, 6)


@pytest.mark.parametrize("batch_norm", [False, True])
@pytest.mark.parametrize("residual", [False, True])
def test_gatedgcnconv_on_cpu_against_fp64_restatement(batch_norm, residual):
    kw = dict(batch_norm=batch_norm, residual=residual)
    EC.check_conv(_graph(60, 60, 4), DEV, 6, 6, 6, **kw)
    EC.check_conv(_graph(60, 60, 4), DEV, 6, 6, 6, seed=1, order="csc", edge_out=False, **kw)
    EC.check_conv(_graph(60, 60, 5), DEV, 8, 3, 5, seed=2, activation=F.elu, **kw)
    EC.check_conv(_graph(30, 80, 6), DEV, 4, 4, 4, seed=3, **kw)                      # n_dst < n_src


def _stack_graph(n=300, seed=13):
    g = SG.small_graph(n, n, seed)
    gen = torch.Generator().manual_seed(seed)
    g.ndata["feat"] = torch.randn(n, 7, generator=gen)
    g.edata["feat"] = torch.randn(g.number_of_edges(), 3, generator=gen)
    return g


def test_gatedgcn_stack_on_cpu_against_fp64_restatement():
    torch.manual_seed(1)
    EC.check_stack(bnn.GatedGCN(7, 3, 4, 6, 3), _stack_graph(), DEV)


def test_stack_permutation_cache_follows_in_place_changes():
    g = _stack_graph(80)
    model = bnn.GatedGCN(7, 3, 4, 6, 2).eval()
    ef = g.edata["feat"]
    first = model.edge_rows(g)
    assert model.edge_rows(g) is first and torch.equal(first, ef[g.csc.eid.long()])   # permuted once per graph and tensor
    assert model.edge_rows(g, "feat") is first and model.edge_rows(g, ef) is first
    with torch.no_grad():
        out0 = model(g)
        ef.mul_(2.0)                                                                # in place: the version moves, the entry is stale
        again = model.edge_rows(g)
        assert again is not first and torch.equal(again, ef[g.csc.eid.long()])
        assert not torch.equal(model(g), out0)
    other = ef.clone()
    assert model.edge_rows(g, other) is not again


def test_refusals():
    g = _graph()
    E = g.number_of_edges()
    k, q, v, c = EC.normal_inputs(40, 40, E, 4, 1)[:4]
    for bad, text in (((k[:-1], q, v, c), "(39, 4)"), ((k, q[:, :3], v, c), "(40, 3)"), ((k, q, v, c[:-1]), f"({E - 1}, 4)"),
                      ((k, q, v.double(), c), "float64"), ((k.long(), q.long(), v.long(), c.long()), "floating point")):
        with pytest.raises(DGLError) as err:
            ops.gated_edge_sum(g, *bad)
        assert text in str(err.value)
    with pytest.raises(ValueError, match="order"):
        ops.gated_edge_sum(g, k, q, v, c, order="coo")
    for eps in (-1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="eps"):
            ops.gated_edge_sum(g, k, q, v, c, eps=eps)
    conv, model = bnn.GatedGCNConv(4, 4, 4), bnn.GatedGCN(7, 3, 4, 6, 2)
    with pytest.raises(ValueError, match="edge_feat"):
        conv(g, k, c[:-1])
    sg = _stack_graph(40)
    with pytest.raises(ValueError, match="each block has its own edges"):
        model([sg, sg])
    with pytest.raises(ValueError, match="one row per edge"):
        model(sg, edge_feats=sg.edata["feat"][:-1])
    g.halo = object()                                                       # a partition's block carries a halo plan
    with pytest.raises(ValueError, match="partition"):
        ops.gated_edge_sum(g, k, q, v, c)
    with pytest.raises(ValueError, match="halo"):
        conv(g, k, c)
    with pytest.raises(ValueError, match="build_gatedgcn_clustered"):
        workloads.build_gatedgcn("proteins", DEV)                           # the edge stream of S-proteins does not fit full-batch
    with pytest.raises(ValueError, match="serve"):
        workloads.build_gatedgcn("cora", DEV)


# ------------------------------------------------------------------------------------------------ the bounds bite
def test_planted_mistakes_exceed_the_bounds():
    g = _big()
    src, dst = EC.positions(g)
    n_src, n_dst = g.number_of_src_nodes(), g.number_of_dst_nodes()
    assert src.numel() >= 5000
    k, q, v, c, a, b, de = (t.double() for t in EC.normal_inputs(n_src, n_dst, src.numel(), 8, 3))
    bnd = EC.bounds(src, dst, k, q, v, c, a, b, de)
    good = EC.forward64(src, dst, k, q, v, c, True)
    gb = EC.backward64(src, dst, good["e"], v, a, b, de)
    over = lambda x, y, lim: bool(((x - y).abs() > lim).any())
    row = int(torch.argmax(EC.degree_of(dst, n_dst)))
    dropped = EC.forward64(src, dst, k, q, v, c, True, drop_last_of=row)
    assert over(dropped["num"], good["num"], bnd["num"]) and over(dropped["den"], good["den"], bnd["den"]) and over(dropped["out"], good["out"], bnd["out"])
    gate = EC.forward64(src, dst, k, q, v, c, True, gate_error=1e-5)
    assert over(gate["num"], good["num"], bnd["num"]) and over(gate["den"], good["den"], bnd["den"])
    late = EC.forward64(src, dst, k, q, v, c, True, c_late=True)
    assert over(late["e"], good["e"], bnd["e"]) and over(late["out"], good["out"], bnd["out"])
    nde = EC.backward64(src, dst, good["e"], v, a, b, de, ignore_de=True)
    for name in ("ds", "dk", "dq"):
        assert over(nde[name], gb[name], bnd[name]), name
    for name in ("ds", "dk", "dq", "dv"):                                    # and the restatement itself is inside them
        assert not over(gb[name], gb[name], bnd[name])


def test_build_gatedgcn_step_on_cpu_tensors():
    wl = workloads.build_gatedgcn("arxiv", DEV, scale=0.002, drop=False)
    assert wl.graph.edata["feat"].shape == (wl.n_edges, 8) and "GatedGCN" in wl.describe
    losses = [float(wl.step()[0].detach()) for _ in range(3)]
    assert all(np.isfinite(x) for x in losses) and losses[-1] < losses[0]
    assert all(p.grad is not None for n, p in wl.model.named_parameters() if "convs.2.bn_edge" not in n)
