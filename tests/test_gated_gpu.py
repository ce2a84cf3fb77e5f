"""Gated aggregation on the MI355X: the three sweeps of csrc/spmm_gate.hip against the float64 restatement (tests/gated_cases.py) - entry
for entry in the contract's three exact regimes (gates 1, 0 and 0.5 on integer-valued operands, whose sums are exact in float32 whatever
their order), the gate's own error read back through a one-edge graph, and under bounds derived from row lengths and rounding counts on
seeded normal inputs - the kernel form against the tensor form, `nn.ResGatedGraphConv` and `nn.ResGatedGCN` against their float64
restatements under the suite's own criteria (tests/parity_cases.py), and the steps of `workloads.build_gated`.

Largest error seen as a fraction of its derived bound (run with -s to print them): DESIGN §8 "Gated graph convolution"."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bot_amd import _C, ops, workloads
from bot_amd import nn as bnn
from bot_amd.errors import DGLError
from bot_amd.sampling import MultiLayerNeighborSampler, NodeDataLoader, sample_block
from tests import block_cases as BC
from tests import gated_cases as GC
from tests import sage_cases as SG

pytestmark = pytest.mark.gpu
DEV = "cuda"
# 1 the smallest; 3, 5 odd widths, 4-byte lanes; 4, 40, 64 one group of 8 / 16 lanes; 65 an odd width beyond a wavefront of 4-byte lanes
# (tiles); 256 the workload's; 1000 walks tiles of 16-byte lanes
WIDTHS = (1, 3, 4, 5, 40, 64, 65, 256, 1000)
WORST = {}
U = GC.U


@functools.lru_cache(maxsize=None)
def _graphs():
    """(name, graph on the device): 1 / 63 / 64 / 65 square rows with isolated rows and parallel edges, chunk = 4 variants (long rows in
    both directions: the workspace and the combine at small sizes), and a block with n_src > n_dst."""
    out = [(f"square{n}", SG.small_graph(n, n, n).to(DEV)) for n in (1, 63, 64, 65)]
    out.append(("long65", SG.small_graph(65, 65, 70, chunk=4).to(DEV)))
    out.append(("block", SG.small_graph(63, 200, 71).to(DEV)))
    out.append(("longblock", SG.small_graph(64, 130, 72, chunk=4).to(DEV)))
    for i in (4, 6):
        assert out[i][1].csc.n_long > 0 and out[i][1].csr.n_long > 0
    assert out[0][1].csc.n_long == 0
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _hub():
    from tests.test_subgraph_gpu import _hub_graph
    g = _hub_graph()
    assert int(np.diff(g.csc.indptr.cpu().numpy()).max()) > 2048 and g.csc.n_long > 0 and g.csr.n_long > 0
    return g


def _slab(t, pad, fill=7.0):
    """A device view of the [n, F] tensor `t` whose rows sit in a buffer `pad` floats wider (row stride F + pad), and the buffer."""
    n, w = t.shape
    buf = torch.full((n, w + pad), fill, dtype=t.dtype, device=DEV)
    buf[:, :w].copy_(t.to(DEV))
    return buf[:, :w], buf


def _merged(q, v):
    """q and v as the two column blocks of ONE [n_src, 2F] matrix, the layer's packing."""
    buf = torch.cat((q, v), dim=1).to(DEV)
    Fw = q.shape[1]
    return buf[:, :Fw], buf[:, Fw:]


def _same_bytes(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _eq(got, want):
    return np.array_equal(got.detach().cpu().double().numpy(), want.numpy())


def _check_exact(g, Fw, pad, seed, lim=8):
    """The three entry points in the three exact regimes, entry for entry; strided operands and outputs with `pad` (pad < 0: q and v as
    the two blocks of one merged matrix)."""
    n_src, n_dst = g.number_of_src_nodes(), g.number_of_dst_nodes()
    csc, csr = g.csc, g.csr
    q, v, a = GC.integer_inputs(n_src, n_dst, Fw, seed, lim)
    if pad < 0:
        (qd, vd), pad = _merged(q, v), 0
    else:
        qd, vd = _slab(q, pad)[0], _slab(v, pad)[0]
    ad = _slab(a, pad)[0]
    deg = np.diff(csc.indptr.cpu().numpy()).astype(np.float32).reshape(-1, 1)
    for regime, kval, qq in (("one", 128.0, qd), ("zero", -128.0, qd), ("half", 0.0, torch.zeros_like(qd))):
        want_out, want_dk, want_dq, want_dv = GC.exact_reference(g, regime, v, a)
        kd = _slab(torch.full((n_dst, Fw), kval), pad)[0]
        o_view, o_buf = _slab(torch.full((n_dst, Fw), 9.0), pad, 9.0)
        out, den = _C.spmm_gate(csc, kd, qq, vd, out=o_view if pad else None)
        assert den is None and "spmm_gate_kernel<0," in _C._lib.bot_last_kernel().decode()
        assert _eq(out, want_out), (regime, Fw, pad)
        assert _same_bytes(_C.spmm_gate(csc, kd, qq, vd)[0], out)                  # the same bytes on a second call
        if regime == "one":                  # normalised at gates 1: float32(num) / (float32(deg) + eps), bit for bit; den is the degree
            d_view, d_buf = _slab(torch.full((n_dst, Fw), 9.0), pad, 9.0)
            for eps in (1e-6, 0.5):
                on, dn = _C.spmm_gate(csc, kd, qq, vd, normalize=True, eps=eps, den=d_view if pad else None)
                assert "spmm_gate_kernel<1," in _C._lib.bot_last_kernel().decode()
                num32 = want_out.numpy().astype(np.float32)
                want_n = np.where(deg > 0, num32 / (deg + np.float32(eps)), np.float32(0))
                assert np.array_equal(on.cpu().numpy().view(np.int32), want_n.astype(np.float32).view(np.int32)), (Fw, pad, eps)
                assert np.array_equal(dn.cpu().numpy(), np.broadcast_to(deg, dn.shape))
            if pad:
                assert bool((d_buf[:, Fw:] == 9.0).all())
        k_view, k_buf = _slab(torch.full((n_dst, Fw), 9.0), pad, 9.0)
        dk = _C.spmm_gate_bwd_dst(csc, kd, qq, vd, ad, out=k_view if pad else None)
        assert "spmm_gate_bwd_dst_kernel<0," in _C._lib.bot_last_kernel().decode()
        assert _eq(dk, want_dk), (regime, Fw, pad)
        assert _same_bytes(_C.spmm_gate_bwd_dst(csc, kd, qq, vd, ad), dk)
        zero_b = torch.zeros((n_dst, Fw), device=DEV)                              # b = 0 runs the normalised instance: the same values
        assert _eq(_C.spmm_gate_bwd_dst(csc, kd, qq, vd, ad, zero_b), want_dk)
        assert "spmm_gate_bwd_dst_kernel<1," in _C._lib.bot_last_kernel().decode()
        q_view, q_buf = _slab(torch.full((n_src, Fw), 9.0), pad, 9.0)
        v_view, v_buf = _slab(torch.full((n_src, Fw), 9.0), pad, 9.0)
        dq, dv = _C.spmm_gate_bwd_src(csr, kd, qq, vd, ad, out_dq=q_view if pad else None, out_dv=v_view if pad else None)
        assert "spmm_gate_bwd_src_kernel<0," in _C._lib.bot_last_kernel().decode()
        assert _eq(dq, want_dq) and _eq(dv, want_dv), (regime, Fw, pad)
        dq2, dv2 = _C.spmm_gate_bwd_src(csr, kd, qq, vd, ad, zero_b)
        assert _eq(dq2, want_dq) and _eq(dv2, want_dv) and "spmm_gate_bwd_src_kernel<1," in _C._lib.bot_last_kernel().decode()
        only_q, none = _C.spmm_gate_bwd_src(csr, kd, qq, vd, ad, want_dv=False)     # NULL outputs: each alone gives the same bytes
        none2, only_v = _C.spmm_gate_bwd_src(csr, kd, qq, vd, ad, want_dq=False)
        assert none is None and none2 is None and _same_bytes(only_q, dq) and _same_bytes(only_v, dv)
        both = torch.full((n_src, 2 * Fw), 9.0, device=DEV)                        # one [n_src, 2F] gradient for the merged projection
        _C.spmm_gate_bwd_src(csr, kd, qq, vd, ad, out_dq=both[:, :Fw], out_dv=both[:, Fw:])
        assert _same_bytes(both[:, :Fw], dq) and _same_bytes(both[:, Fw:], dv)
        if pad:                                                                     # nothing is written beyond a strided row
            assert all(bool((b[:, Fw:] == 9.0).all()) for b in (o_buf, k_buf, q_buf, v_buf))


# ------------------------------------------------------------------------------------------------ 1. exact
@pytest.mark.parametrize("Fw", WIDTHS)
def test_exact_regimes_entry_for_entry(Fw):
    for i, (name, g) in enumerate(_graphs()):
        for pad in (0, 3, 4, -1):
            _check_exact(g, Fw, pad, seed=17 * i + Fw + pad)


def test_exact_regimes_on_the_hub_graph():
    """Rows above 2 048 in-edges at the default chunk; the ranges are shrunk so that every sum's absolute terms stay below 2^22."""
    _check_exact(_hub(), 5, 0, seed=3, lim=2)


def test_gate_error_read_back_through_a_one_edge_graph():
    """g = out of a one-edge row with v = 1; gbar(s) is the same quotient as g(-s) (e / (1 + e) or 1 / (1 + e)), read at -s; g' = dk of
    the same row with v = a = 1.  Against float64 over s in [-87, 87]: at most 8 U relative for g and gbar (4 U the exponential, 2 U more
    where its error reaches 1 + e, 1 U the addition, 1 U the division), 17 U for the rounded product g'.  The exact regimes bit for bit."""
    import bot_amd
    n, Fw = 8192, 4
    ids = torch.arange(n)
    g = bot_amd.Graph(ids, ids, n).to(DEV)
    s = torch.linspace(-87.0, 87.0, n * Fw, dtype=torch.float64).float().view(n, Fw)
    s[0] = torch.tensor([0.0, 105.0, -105.0, 120.0])
    s[1] = torch.tensor([-120.0, 87.0, -87.0, 1000.0])
    sd, zero, one = s.to(DEV), torch.zeros((n, Fw), device=DEV), torch.ones((n, Fw), device=DEV)
    want_g, want_gbar = GC.gate64(s.double())
    got_g = _C.spmm_gate(g.csc, zero, sd, one)[0].cpu().double()
    got_gbar = _C.spmm_gate(g.csc, zero, -sd, one)[0].cpu().double()
    got_gp = _C.spmm_gate_bwd_dst(g.csc, zero, sd, one, one).cpu().double()
    assert got_g[0].tolist() == [0.5, 1.0, 0.0, 1.0] and got_gbar[0].tolist() == [0.5, 0.0, 1.0, 0.0] and got_gp[0].tolist() == [0.25, 0.0, 0.0, 0.0]
    assert got_g[1, 0] == 0.0 and got_g[1, 3] == 1.0 and got_gp[1, 0] == 0.0 and got_gp[1, 3] == 0.0
    body = slice(2, None)
    rel = lambda a, b: float(((a - b).abs() / b)[body].max() / U)
    eg, egbar, egp = rel(got_g, want_g), rel(got_gbar, want_gbar), rel(got_gp, want_g * want_gbar)
    print(f"gate error over s in [-87, 87] in units of 2^-24: g {eg:.3f}, gbar {egbar:.3f}, g' {egp:.3f} (bounds {GC.GATE_UNITS}, {GC.GATE_UNITS}, {2 * GC.GATE_UNITS + 1})")
    assert eg <= GC.GATE_UNITS and egbar <= GC.GATE_UNITS and egp <= 2 * GC.GATE_UNITS + 1
    dq, dv = _C.spmm_gate_bwd_src(g.csr, zero, sd, one, one)                       # the source-side sweep forms the same gates
    assert _same_bytes(dq, got_gp.float().to(DEV)) and _same_bytes(dv, got_g.float().to(DEV))


# ------------------------------------------------------------------------------------------------ 2. rounded, and the two forms
def _check_kernels_with_b(g, Fw, seed):
    """The two backward sweeps with a given (a, b) - the normalised instances - against float64 under the derived bounds."""
    src, dst = GC.positions(g)
    k, q, v, a, b = GC.normal_inputs(g.number_of_src_nodes(), g.number_of_dst_nodes(), Fw, seed)
    want, _ = GC.backward64(src, dst, *(t.double() for t in (k, q, v, a, b)))
    bnd = GC.bounds(src, dst, *(t.double() for t in (k, q, v, a, b)))
    kd, ad, bd = k.to(DEV), a.to(DEV), b.to(DEV)
    qd, vd = _merged(q, v)
    dk = _C.spmm_gate_bwd_dst(g.csc, kd, qd, vd, ad, bd)
    dq, dv = _C.spmm_gate_bwd_src(g.csr, kd, qd, vd, ad, bd)
    fwd = GC.forward64(src, dst, k.double(), q.double(), v.double(), True, 1e-6)
    out, den = _C.spmm_gate(g.csc, kd, qd, vd, normalize=True, eps=1e-6)
    for name, x, y in (("dk", dk, want[0]), ("dq", dq, want[1]), ("dv", dv, want[2]), ("den", den, fwd["den"]), ("out", out, fwd["out"])):
        err = (x.cpu().double() - y).abs()
        frac = GC._record(WORST, "kernel with b " + name, err, bnd[name])
        assert bool((err <= bnd[name]).all()), (name, Fw, frac)


@pytest.mark.parametrize("Fw", WIDTHS)
def test_kernel_and_tensor_forms_against_fp64_under_derived_bounds(Fw):
    for i in (3, 4, 5, 6):
        name, g = _graphs()[i]
        for normalize in (False, True):
            got_k, bnd = GC.check_op(g, DEV, Fw, seed=i + Fw, impl="kernel", normalize=normalize, worst=WORST)
            got_t, bnd_t = GC.check_op(g, DEV, Fw, seed=i + Fw, impl="tensor", normalize=normalize, worst=WORST)
            if not normalize:
                for a, b, lk, lt in zip(got_k, got_t, bnd, bnd_t):              # the two forms agree within the sum of their bounds
                    assert bool(((a - b).abs() <= lk + lt).all())
        _check_kernels_with_b(g, Fw, seed=i + 2 * Fw)
    print("largest error / bound so far:", {k: round(v, 4) for k, v in sorted(WORST.items())})
    assert all(v <= 1.0 for v in WORST.values())


def test_hub_graph_against_fp64_under_derived_bounds():
    """Rows above 2 048 edges in both directions: the output and the three gradients.  (The normalised instances' long rows: the
    chunk = 4 graphs above.)"""
    GC.check_op(_hub(), DEV, 5, seed=2, impl="kernel", worst=WORST)
    print("largest error / bound so far:", {k: round(v, 4) for k, v in sorted(WORST.items())})
    assert all(v <= 1.0 for v in WORST.values())


def test_impl_selection_is_read_at_call_time(monkeypatch):
    g = _graphs()[5][1]
    monkeypatch.setenv("BOT_GATE", "tensor")
    calls = []
    real = _C.spmm_gate
    monkeypatch.setattr(_C, "spmm_gate", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    GC.check_op(g, DEV, 5, seed=2)
    assert calls == []
    GC.check_op(g, DEV, 5, seed=2, impl="kernel")                    # the argument wins over the variable
    assert calls == [1]
    monkeypatch.delenv("BOT_GATE")
    GC.check_op(g, DEV, 5, seed=2)
    assert len(calls) == (2 if ops.gate_default_impl == "kernel" else 1)


def test_needed_gradients_only_and_nothing_kept_under_no_grad(monkeypatch):
    calls = []
    real_dst, real_src = _C.spmm_gate_bwd_dst, _C.spmm_gate_bwd_src
    monkeypatch.setattr(_C, "spmm_gate_bwd_dst", lambda *a, **k: (calls.append(("dst",)), real_dst(*a, **k))[1])
    monkeypatch.setattr(_C, "spmm_gate_bwd_src", lambda *a, **k: (calls.append(("src", k["want_dq"], k["want_dv"])), real_src(*a, **k))[1])
    x = [torch.randn(20, 8, device=DEV), torch.randn(30, 8, device=DEV), torch.randn(30, 8, device=DEV)]
    full = None
    for normalize in (False, True):
        for need, seen in (((True, True, True), [("dst",), ("src", True, True)]), ((True, False, False), [("dst",)]),
                           ((False, True, False), [("src", True, False)]), ((False, False, True), [("src", False, True)])):
            g2 = SG.small_graph(20, 30, 8).to(DEV)
            calls.clear()
            leaves = [t.clone().requires_grad_(r) for t, r in zip(x, need)]
            ops.gated_sum(g2, *leaves, normalize=normalize, impl="kernel").sum().backward()
            assert calls == seen and (g2._csr is None) == (need == (True, False, False))   # the CSR is built only for dq or dv
            grads = [t.grad for t in leaves]
            if all(need):
                full = grads
            else:                                                    # a subset gives the bytes of the full backward
                assert all(a is None or _same_bytes(a, b) for a, b in zip(grads, full))
    g2 = SG.small_graph(20, 30, 8).to(DEV)
    with torch.no_grad():
        out = ops.gated_sum(g2, *x, normalize=True, impl="kernel")
    assert out.grad_fn is None and not out.requires_grad


# ------------------------------------------------------------------------------------------------ 3. the layer
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


@functools.lru_cache(maxsize=None)
def _subgraph():
    g = _parent()
    nodes = torch.randperm(g.number_of_nodes(), generator=torch.Generator().manual_seed(4))[:1500].sort().values
    return g.subgraph(nodes.to(DEV))


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("root_weight", [False, True])
def test_resgatedgraphconv_against_fp64_restatement(normalize, root_weight):
    kw = dict(normalize=normalize, root_weight=root_weight)
    GC.check_conv(_parent(), DEV, 8, 5, **kw)
    GC.check_conv(_parent(), DEV, 8, 64, seed=1, bias=False, activation=F.elu, **kw)
    GC.check_conv(_subgraph(), DEV, 8, 6, seed=2, **kw)
    b = _block()
    GC.check_conv(b, DEV, (8, 6), 8, seed=3, pair=True, **kw)
    GC.check_conv(b, DEV, 8, 4, seed=4, **kw)


def test_merged_projection_reaches_the_sweeps_as_one_matrix():
    """Query and value come out of ONE product (at this width `gemm.linear_blocks`, where the fp16-halves GEMM pays) and reach
    `ops.gated_sum` as the two column blocks of one [n, 2F] matrix, which the sweeps gather as one row."""
    from bot_amd import gemm
    g = _parent()
    seen = []
    real = ops.gated_sum
    conv = GC.make_conv(128, 128, 5, normalize=True).to(DEV)
    x = torch.randn(g.number_of_nodes(), 128, device=DEV)
    old = gemm.MIN_ROWS
    gemm.MIN_ROWS = 1024
    try:
        ops.gated_sum = lambda gr, k, q, v, **kw: (seen.append((q, v)), real(gr, k, q, v, **kw))[1]
        out = conv(g, x)
    finally:
        ops.gated_sum, gemm.MIN_ROWS = real, old
    q, v = seen[0]
    assert q.shape == (g.number_of_nodes(), 128) and q.stride() == (256, 1) and v.stride() == (256, 1)
    assert v.data_ptr() == q.data_ptr() + 128 * 4 and bool(torch.isfinite(out).all())
    GC.check_conv(g, DEV, 128, 128, seed=5, normalize=True)


# ------------------------------------------------------------------------------------------------ 4. the stack and the recipes
def test_resgatedgcn_stack_against_fp64_restatement():
    g = _parent()
    torch.manual_seed(3)
    model = bnn.ResGatedGCN(8, 5, 6, 3, F.relu, norm="batch", dropout=0.5, normalize=True)
    GC.check_stack(model, g, g.ndata["feat"].cpu(), DEV)
    nids = torch.randperm(g.number_of_nodes(), generator=torch.Generator().manual_seed(3))[:600]
    _, _, blocks = next(iter(NodeDataLoader(g, nids, MultiLayerNeighborSampler([5, 7, 9]), batch_size=600, seed=4)))
    model2 = bnn.ResGatedGCN(8, 5, 6, 3, F.relu)
    GC.check_stack(model2, blocks, blocks[0].srcdata["feat"].cpu(), DEV)


def _losses(step, n=5):
    torch.manual_seed(0)
    out = []
    for _ in range(n):
        out.append(float(torch.as_tensor(step()).detach()))
    assert all(np.isfinite(v) for v in out) and out[-1] < out[0], out
    return out


def test_build_gated_full_batch_steps():
    wl = workloads.build_gated("cora", DEV, drop=False)
    _losses(lambda: wl.step()[0])
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in wl.model.parameters())


def test_build_gated_sampled_epochs():
    wl = workloads.build_gated("cora", DEV, sampled=True, drop=False)
    _losses(wl.epoch, 2)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in wl.model.parameters())


def test_gated_under_subgraph_steps():
    from bot_amd import minibatch
    wl = workloads.build_gated("cora", DEV, drop=False)
    ds, g = wl.dataset, wl.graph
    n = g.number_of_nodes()
    roles = minibatch.node_roles(n, ds.train_idx, ds.val_idx, ds.test_idx)
    g.ndata["feat"] = ds.feat
    sub = g.subgraph(torch.arange(0, n, 2, device=DEV))
    res = minibatch.subgraph_step(wl.model, sub, wl.optimizer, ds.labels, roles, step_kw=wl.step_kw)
    assert res is not None and np.isfinite(float(res[0].detach()))


# ------------------------------------------------------------------------------------------------ 5. errors
def test_error_paths():
    name, g = _graphs()[3]
    n = g.number_of_nodes()
    x = torch.randn(n, 8, device=DEV)
    assert ops.gated_sum(g, x, x, x).shape == (n, 8)
    for bad, text in (((x[:-1], x, x), f"({n - 1}, 8)"), ((x, x[:, :4], x), f"({n}, 4)"), ((x, x, x.cpu()), "cpu"), ((x, x, x.double()), "float64")):
        with pytest.raises(DGLError) as err:
            ops.gated_sum(g, *bad)
        assert text in str(err.value)
    part = BC.parent_graph(DEV, n=200, e_raw=1500, seed=7)
    part.halo = object()                                              # a partition's block carries a halo plan
    with pytest.raises(ValueError, match="partition"):
        ops.gated_sum(part, *(torch.randn(200, 4, device=DEV) for _ in range(3)))
    model = bnn.ResGatedGCN(8, 5, 6, 2, F.relu).to(DEV)
    p = _parent()
    with pytest.raises(ValueError, match="edge_weight"):
        model(p, p.ndata["feat"], edge_weight=torch.ones(p.number_of_edges(), device=DEV))
    with pytest.raises(_C.BotKernelError, match="unit inner stride"):
        _C.spmm_gate(g.csc, x.t().contiguous().t(), x, x)
    out = bnn.ResGatedGraphConv(8, 4, root_weight=False, bias=False).to(DEV)(g, x)
    assert bool((out[g.in_degrees() == 0] == 0).all())                # every fifth node of the graph has no in-edges
