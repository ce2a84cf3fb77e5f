"""Dot-product attention with edge features on the MI355X: the two sweeps of csrc/dot_attn_edge.hip against the float64 restatements
(tests/dot_attn_edge_cases.py) - bit for bit in the exact regimes (qe = 0 / uniform, ef = 0 against the plain sweeps' bytes, one-hot
with parallel edges that only their edge features separate) and under the derived bounds on seeded normal inputs, at kernel level with
a given qe and at op level against PyG's formula - the kernel form against the tensor form, the fall-backs, `nn.EdgeTransformerConv` and
`nn.EdgeUniMP` against their float64 restatements under the suite's own criteria (tests/parity_cases.py), and the steps of
`workloads.build_unimp_edge`.

ef = 0 against the plain sweeps, bit for bit: the edge sweeps narrow their vectors until D / VEC >= K, and the order of the logit's sum
is fixed per instance, so where that narrowing happens ((8, 32, 16): 4 -> 2, (1, 16, 16): 4 -> 1) the plain sweeps are handed a q at
a storage offset that makes them pick the same instance (common.h pick_vec), and the bytes are compared all the same.

Largest error seen as a fraction of its derived bound (run with -s to print them): see README "Dot-product attention with edge features"."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bot_amd import _C, ops, workloads
from bot_amd import nn as bnn
from bot_amd.sampling import MultiLayerNeighborSampler, NodeDataLoader
from tests import dot_attn_cases as DC
from tests import dot_attn_edge_cases as EC
from tests import gatv2_cases as GC
from tests import test_dot_attn_gpu as PG

DEV = "cuda"
# (3, 5, 3) odd width, 4-byte lanes, heads that end inside a group; (2, 64, 8) heads that are whole spans of lanes; (8, 32, 16) VEC has to
# drop from 4 to 2; (4, 65, 8) heads straddling 64-lane chunks; (3, 250, 8) six chunks; (8, 250, 1) several head tiles; (1, 16, 16) every
# slot owns a column (VEC = 1)
CASES = ((3, 5, 3), (2, 64, 8), (8, 32, 16), (4, 65, 8), (3, 250, 8), (8, 250, 1), (1, 16, 16))
WORST = {}
U = DC.U
_same, _slab, _held = PG._same, PG._slab, PG._held


@functools.lru_cache(maxsize=None)
def _graphs():
    """test_dot_attn_gpu.graph_specs()' seven graphs.  Their edge ids are NOT their CSC positions."""
    out = PG._graphs()
    assert not torch.equal(EC.eid_of_positions(out[1][1]), torch.arange(out[1][1].number_of_edges()))
    return out


def _edge_vec(D, K):
    return next(w for w in (4, 2, 1) if D % w == 0 and D // w >= K)


def _plain_vec(D):
    return next(w for w in (4, 2, 1) if D % w == 0)


def _vec_for(g, D, K, pad):
    """The vector width the edge sweeps pick for slabs `pad` floats wider than their rows (a one-row operand has no row stride)."""
    return _edge_vec(D, K) if pad % 4 == 0 or g.number_of_src_nodes() == 1 else 1


def _note(name, got, want, bound):
    if got.numel():
        WORST[name] = max(WORST.get(name, 0.0), float(((got.detach().cpu().double() - want).abs() / bound.clamp(min=1e-300)).max()))


def _run_sweeps(g, q, k, v, dout, qe, ef, daef, scale, keep, p, pad):
    """The two new entry points (and the plain sweep over the sources) on possibly strided operands and outputs -> a dict of results;
    checks the instances that ran, that two calls give the same bytes, that each gradient alone gives the same bytes, and that nothing
    is written beyond a strided row.  ef: POSITION order."""
    n_src, n_dst, E = g.number_of_src_nodes(), g.number_of_dst_nodes(), g.number_of_edges()
    H, D, K = q.shape[1], q.shape[2], ef.shape[1]
    csc, csr = g.csc, g.csr
    qd, kd, vd, dd, qed, efd, dad = (_slab(t, pad)[0] for t in (q, k, v, dout, qe, ef, daef))
    bits = None if keep is None else ops.pack_keep(keep.to(DEV))
    nine = lambda *shape: _slab(torch.full(shape, 9.0), pad, 9.0)
    (o_out, o_buf), (l_out, l_buf), (a_out, a_buf) = nine(n_dst, H, D), nine(n_dst, H), nine(n_dst, H, K)
    give = lambda t: t if pad else None
    out, lse, aef = _C.dot_attn_edge(csc, qd, kd, vd, qed, efd, scale, bits, p, out=give(o_out), lse=give(l_out), aef=give(a_out))
    name = _C._lib.bot_last_kernel().decode()
    assert f"dot_attn_edge_kernel<{_vec_for(g, D, K, pad)}," in name, name
    again = _C.dot_attn_edge(csc, qd, kd, vd, qed, efd, scale, bits, p)
    assert all(_same(a, b) for a, b in zip(again, (out, lse, aef)))
    if keep is None:                                                            # keep = all ones and keep = NULL: the same bytes
        ones = torch.full((E,), -1, dtype=torch.int32, device=DEV)
        assert all(_same(a, b) for a, b in zip(_C.dot_attn_edge(csc, qd, kd, vd, qed, efd, scale, ones, 0.0), (out, lse, aef)))
    (dq_out, dq_buf), (de_out, de_buf) = nine(n_dst, H, D), nine(n_dst, H, K)
    bwd = lambda **kw: _C.dot_attn_edge_bwd_dst(csc, qd, kd, vd, qed, efd, scale, bits, p, dd, dad, out, lse, aef, **kw)
    dq, dqe, pw, ds = bwd(dq=give(dq_out), dqe=give(de_out))
    assert "dot_attn_edge_bwd_dst_kernel<" in _C._lib.bot_last_kernel().decode()
    dq2, dqe2, pw2, ds2 = bwd()
    dq3, n1, pw3, ds3 = bwd(want_dqe=False)
    n2, dqe3, pw4, ds4 = bwd(want_dq=False)
    n3, n4, pw5, ds5 = bwd(want_dq=False, want_dqe=False)
    assert n1 is None and n2 is None and n3 is None and n4 is None
    assert all(_same(a, dq) for a in (dq2, dq3)) and all(_same(a, dqe) for a in (dqe2, dqe3))
    assert all(_same(a, pw) for a in (pw2, pw3, pw4, pw5)) and all(_same(a, ds) for a in (ds2, ds3, ds4, ds5))
    dk, dv = _C.dot_attn_bwd_src(csr, g.csr2csc, qd, dd, pw, ds, scale)           # the plain sweep over the sources, unchanged
    if pad:                                                                     # nothing is written beyond a strided row
        for buf, w in ((o_buf, H * D), (l_buf, H), (a_buf, H * K), (dq_buf, H * D), (de_buf, H * K)):
            assert bool((buf[:, w:] == 9.0).all())
    return dict(out=out, lse=lse, aef=aef, dq=dq, dqe=dqe, p=pw, ds=ds, dk=dk, dv=dv)


def _plain(g, q, k, v, dout, scale, keep, p, vec):
    """The plain sweeps' bytes at the vector width `vec`: q sits at a storage offset that makes pick_vec choose it (8 bytes off a 16-byte
    boundary: 2; 4 bytes off: 1)."""
    off = {4: 0, 2: 2, 1: 1}[vec] if vec != _plain_vec(q.shape[2]) else 0
    kd, vd, dd = (t.to(DEV) for t in (k, v, dout))
    qbuf = torch.zeros(q.numel() + 4, device=DEV)
    qd = qbuf[off:off + q.numel()].view(q.shape)
    qd.copy_(q)
    assert qd.data_ptr() % 16 == 4 * off
    bits = None if keep is None else ops.pack_keep(keep.to(DEV))
    out, lse = _C.dot_attn(g.csc, qd, kd, vd, scale, bits, p)
    assert f"dot_attn_kernel<0,{vec}," in _C._lib.bot_last_kernel().decode()
    dq, pw, ds = _C.dot_attn_bwd_dst(g.csc, qd, kd, vd, scale, bits, p, dd, out, lse)
    assert f"dot_attn_bwd_dst_kernel<0,{vec}," in _C._lib.bot_last_kernel().decode()
    return dict(out=out, lse=lse, dq=dq, p=pw, ds=ds)


# ------------------------------------------------------------------------------------------------ 1. exact regimes
def _check_qe_zero(g, H, D, K, seed, pad, p=0.0, lim=8):
    """qe = 0 and q = 0 (the uniform regime) with integer-valued v and ef: out and lse are `_C.dot_attn`'s bytes, out = c float32(sum of the
    kept v) / float32(deg) and aef = c float32(sum of the kept ef) / float32(deg), bit for bit."""
    (q, k, v, dout), src, dst = DC.uniform_inputs(g, H, D, seed, lim)
    n_dst, E = g.number_of_dst_nodes(), src.numel()
    rng = np.random.default_rng(seed + 5)
    ef, daef = DC._ints(rng, -lim, lim, (E, K)), DC._ints(rng, -lim, lim, (n_dst, H, K))
    keep = DC.draw_keep(E, H, p, seed + 1) if p > 0 else None
    res = _run_sweeps(g, q, k, v, dout, torch.zeros(n_dst, H, K), ef, daef, D ** -0.5, keep, p, pad)
    plain = _plain(g, q, k, v, dout, D ** -0.5, keep, p, _plain_vec(D))
    assert _same(res["out"], plain["out"]) and _same(res["lse"], plain["lse"]), (H, D, K, pad, p)
    kd = 1.0 if keep is None else keep.double().unsqueeze(-1)
    deg = GC.degree_of(dst, n_dst).view(-1, 1, 1).clamp(min=1).float()
    c = 1.0 / (1.0 - p)                                                          # p is 0 or 0.5: the factor is exact
    tot_v = torch.zeros(n_dst, H, D, dtype=torch.float64).index_add_(0, dst, v.double()[src] * kd)
    tot_e = torch.zeros(n_dst, H, K, dtype=torch.float64).index_add_(0, dst, ef.double().unsqueeze(1).expand(-1, H, -1) * kd)
    assert torch.equal(res["out"].cpu(), c * (tot_v.float() / deg)) and torch.equal(res["aef"].cpu(), c * (tot_e.float() / deg)), (H, D, K, pad, p)


def _check_qe_zero_general(g, H, D, K, seed, pad, p=0.0):
    """qe = 0 with seeded normal q and k and integer-valued v, ef: the edge term adds zeros to the logit, so out and lse are the plain
    forward's bytes (same instance: module docstring)."""
    src, dst = EC.positions(g)
    n_src, n_dst, E = g.number_of_src_nodes(), g.number_of_dst_nodes(), src.numel()
    q, k, _, dout, _, _, _, daef = EC.normal_inputs(n_src, n_dst, E, H, D, K, seed)
    rng = np.random.default_rng(seed + 9)
    v, ef = DC._ints(rng, -8, 8, (n_src, H, D)), DC._ints(rng, -8, 8, (E, K))
    keep = DC.draw_keep(E, H, p, seed + 1) if p > 0 else None
    res = _run_sweeps(g, q, k, v, dout, torch.zeros(n_dst, H, K), ef, daef, D ** -0.5, keep, p, pad)
    plain = _plain(g, q, k, v, dout, D ** -0.5, keep, p, _vec_for(g, D, K, pad))
    assert _same(res["out"], plain["out"]) and _same(res["lse"], plain["lse"]), (H, D, K, pad, p)


def _check_ef_zero(g, H, D, K, seed, pad, p=0.0):
    """ef = 0 on seeded normal inputs: out, lse, p, ds, dq are the plain sweeps' bytes (same instance: module docstring); aef and dqe
    are exact zeros."""
    src, dst = EC.positions(g)
    n_src, n_dst, E = g.number_of_src_nodes(), g.number_of_dst_nodes(), src.numel()
    q, k, v, dout, _, _, qe, daef = EC.normal_inputs(n_src, n_dst, E, H, D, K, seed)
    keep = DC.draw_keep(E, H, p, seed + 1) if p > 0 else None
    res = _run_sweeps(g, q, k, v, dout, qe, torch.zeros(E, K), daef, D ** -0.5, keep, p, pad)
    plain = _plain(g, q, k, v, dout, D ** -0.5, keep, p, _vec_for(g, D, K, pad))
    for n in ("out", "lse", "p", "ds", "dq"):
        assert _same(res[n], plain[n]), (n, H, D, K, pad, p)
    assert bool((res["aef"] == 0).all()) and bool((res["dqe"] == 0).all())


def _check_onehot(g, H, D, K, seed, pad, p=0.0, lim=None):
    """One-hot weights with parallel edges that only their ef rows separate: tests/dot_attn_edge_cases.onehot_inputs."""
    E, n_src = g.number_of_edges(), g.number_of_src_nodes()
    keep = DC.draw_keep(E, H, p, seed + 1) if p > 0 else None
    c = 1.0 / (1.0 - p)
    case = EC.onehot_inputs(g, H, D, K, seed, lim=lim, keep=keep, c=c)
    fwd, bwd, dst = case["fwd"], case["bwd"], case["dst"]
    res = _run_sweeps(g, case["q"], case["k"], case["v"], case["dout"], case["qe"], case["ef"], case["daef"], case["scale"], keep, p, pad)
    assert torch.equal(res["out"].cpu(), case["out32"]) and torch.equal(res["aef"].cpu(), case["aef32"]), (H, D, K, pad, p)
    assert bool(((res["lse"].cpu().double() - fwd["lse"]).abs() <= 3 * U * fwd["lse"].abs()).all())
    one_dst, one_src = DC.exact_entries(case, n_src)
    want, bb = EC.onehot_backward_from_lse(case, res["lse"].cpu(), D, K, c, keep)
    exact = dict(dq=one_dst, dqe=one_dst, p=one_dst[dst], ds=one_dst[dst], dk=one_src, dv=one_src)
    for n in exact:
        _held(res[n], bwd[n], exact[n], None, n)                     # one maximal in-edge: the ideal sums, entry for entry
        _held(res[n], want[n], None, bb[n], n)                       # everywhere: the contract's sums from the float32 lse
        _note("onehot " + n, res[n], want[n], bb[n])


@pytest.mark.gpu
@pytest.mark.parametrize("H,D,K", CASES)
def test_exact_regimes(H, D, K):
    for i, (name, g) in enumerate(_graphs()):
        seed = PG.exact_seed(i, H, D) + K
        for pad, p in ((0, 0.0), (3, 0.0), (4, 0.5)):
            _check_qe_zero(g, H, D, K, seed, pad, p)
            _check_qe_zero_general(g, H, D, K, seed, pad, p)
            _check_ef_zero(g, H, D, K, seed, pad, p)
            _check_onehot(g, H, D, K, seed, pad, p)
    print("largest error / bound so far:", {k: round(v, 4) for k, v in WORST.items() if k.startswith("onehot")})


@pytest.mark.gpu
def test_exact_regimes_on_the_hub_graph():
    """Rows above 2 048 in-edges at the default chunk: the extra workspace plane and both combines at full length."""
    g = PG._hub()
    _check_qe_zero(g, 2, 4, 3, 3, 0, lim=2)
    _check_ef_zero(g, 2, 4, 3, 3, 0)


# ------------------------------------------------------------------------------------------------ 2. rounded: kernel level, op level, forms
def _check_kernel_level(g, H, D, K, seed, pad, p):
    src, dst = EC.positions(g)
    n_src, n_dst, E = g.number_of_src_nodes(), g.number_of_dst_nodes(), src.numel()
    q, k, v, dout, ef, _, qe, daef = EC.normal_inputs(n_src, n_dst, E, H, D, K, seed)
    keep = DC.draw_keep(E, H, p, seed + 1) if p > 0 else None
    c = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    sc = D ** -0.5
    res = _run_sweeps(g, q, k, v, dout, qe, ef, daef, sc, keep, p, pad)
    a64 = [t.double() for t in (q, k, v, ef, qe)]
    fwd = EC.forward64(src, dst, n_dst, *a64, sc, keep, c)
    bwd = EC.backward64(src, dst, n_src, n_dst, *a64, sc, dout.double(), daef.double(), fwd, keep, c)
    fb = EC.forward_bounds(fwd, D, K, c)
    bb = EC.backward_bounds(src, dst, n_src, n_dst, *a64[:4], sc, dout.double(), daef.double(), fwd, bwd, fb, D, K, c)
    for n in ("out", "lse", "aef"):
        _held(res[n], fwd[n], None, fb[n], n)
        _note("kernel " + n, res[n], fwd[n], fb[n])
    for n in ("dq", "dqe", "dk", "dv", "p", "ds"):
        _held(res[n], bwd[n], None, bb[n], n)
        _note("kernel " + n, res[n], bwd[n], bb[n])


@pytest.mark.gpu
@pytest.mark.parametrize("H,D,K", CASES)
def test_kernel_level_against_fp64_under_derived_bounds(H, D, K):
    for i, (name, g) in enumerate(_graphs()):
        for pad, p in ((0, 0.0), (0, 0.25), (3, 0.25)):
            _check_kernel_level(g, H, D, K, i + H * D + K, pad, p)
    print("largest error / bound so far:", {k: round(v, 4) for k, v in WORST.items() if not isinstance(v, dict)})


@pytest.mark.gpu
@pytest.mark.parametrize("H,D,K", CASES)
def test_op_level_and_the_two_forms_against_pyg_in_fp64(H, D, K):
    for i, (name, g) in enumerate(_graphs()):
        for p in (0.0, 0.25):
            wk, wt = WORST.setdefault("op kernel form", {}), WORST.setdefault("op tensor form", {})
            got_k, lim = EC.check_op(g, DEV, H, D, K, seed=i + H * D + K, impl="kernel", p=p, worst=wk)
            assert ops.dot_attn_last_impl == "kernel"
            got_t, _ = EC.check_op(g, DEV, H, D, K, seed=i + H * D + K, impl="tensor", p=p, worst=wt)
            assert ops.dot_attn_last_impl == "tensor"
            for n in got_k:                                              # the two forms against each other: the sum of the two bounds
                assert bool(((got_k[n] - got_t[n]).abs() <= 2 * lim[n]).all()), n
    print("largest error / bound so far:", {k: {a: round(b, 4) for a, b in v.items()} for k, v in WORST.items() if isinstance(v, dict)})


@pytest.mark.gpu
def test_hub_graph_and_a_sampled_block():
    _check_kernel_level(PG._hub(), 2, 4, 3, 2, 0, 0.25)
    b = PG._block()                                                      # a sampled block: its edge ids ARE its positions
    from bot_amd.ops import _csc_edge_rows
    assert _csc_edge_rows(b) is None
    EC.check_op(b, DEV, 4, 16, 8, seed=3, impl="kernel", p=0.25)
    assert ops.dot_attn_last_impl == "kernel"


@pytest.mark.gpu
def test_refusals_and_fall_backs():
    name, g = _graphs()[5]
    n_src, n_dst, E = g.number_of_src_nodes(), g.number_of_dst_nodes(), g.number_of_edges()
    for H, D, K in ((1, 1, 3), (2, 20, 17)):                             # D < K; K = 17: the entry points refuse, the op runs the tensor form
        q, k, v, dout, ef, W, qe, daef = (t.to(DEV) for t in EC.normal_inputs(n_src, n_dst, E, H, D, K, 0))
        if K <= 16:
            with pytest.raises(_C.BotKernelError, match="D >= K"):
                _C.dot_attn_edge(g.csc, q, k, v, qe, ef, 1.0)
        else:
            with pytest.raises(_C.BotKernelError, match="K <= 16"):
                _C.dot_attn_edge(g.csc, q, k, v, qe, ef, 1.0)
        rc = _C._lib.bot_dot_attn_edge_f32(
            g.csc.indptr.data_ptr(), g.csc.indices.data_ptr(), n_dst, E, g.csc.items.data_ptr(), g.csc.n_items, None, None, 0, 0, q.data_ptr(),
            H * D, k.data_ptr(), H * D, v.data_ptr(), H * D, qe.data_ptr(), H * K, ef.data_ptr(), K, H, D, K, 1.0, None, 0.0, dout.data_ptr(), H * D,
            torch.zeros(n_dst, H, device=DEV).data_ptr(), H, daef.data_ptr(), H * K, None, None)
        assert rc == -2
        EC.check_op(g, DEV, H, D, K, seed=1, impl="kernel")
        assert ops.dot_attn_last_impl == "tensor"
    EC.check_op(g, DEV, 3, 5, 3, seed=2, impl="kernel", ef_grad=True)     # ef.requires_grad: the tensor form, which has that gradient
    assert ops.dot_attn_last_impl == "tensor"
    q, k, v, dout, ef, W, _, _ = (t.to(DEV) for t in EC.normal_inputs(n_src, n_dst, E, 3, 5, 3, 4))
    out, a = ops.dot_attention_edge(g, q, k, v, ef, W, return_attention=True)
    assert ops.dot_attn_last_impl == "tensor" and a.shape == (E, 3, 1)
    assert torch.allclose(out, ops.dot_attention_edge(g, q, k, v, ef, W), rtol=1e-4, atol=1e-5) and ops.dot_attn_last_impl == "kernel"
    src, dst = EC.positions(g)
    ref = EC.op_backward64(src, dst, n_src, n_dst, q.cpu().double(), k.cpu().double(), v.cpu().double(),
                           ef.cpu().double()[EC.eid_of_positions(g)], W.cpu().double(), 5 ** -0.5, dout.cpu().double())
    lim = EC.op_bounds(src, dst, n_src, n_dst, q.cpu().double(), k.cpu().double(), v.cpu().double(), ef.cpu().double()[EC.eid_of_positions(g)],
                       W.cpu().double(), 5 ** -0.5, dout.cpu().double(), ref)
    assert bool(((out.cpu().double() - ref["out"]).abs() <= lim["out"]).all())
    keep33 = torch.ones(E, 33, dtype=torch.bool, device=DEV)             # one bit per head: above 32 the op runs the tensor form
    ops.dot_attention_edge(g, torch.randn(n_dst, 33, 2, device=DEV), *(torch.randn(n_src, 33, 2, device=DEV),) * 2, torch.randn(E, 2, device=DEV),
                           torch.randn(66, 2, device=DEV), keep=keep33, p=0.5)
    assert ops.dot_attn_last_impl == "tensor"


@pytest.mark.gpu
def test_autograd_computes_each_gradient_only_when_asked(monkeypatch):
    calls = []
    real_dst, real_src = _C.dot_attn_edge_bwd_dst, _C.dot_attn_bwd_src
    monkeypatch.setattr(_C, "dot_attn_edge_bwd_dst", lambda *a, **k: (calls.append(("dst", k["want_dq"], k["want_dqe"])), real_dst(*a, **k))[1])
    monkeypatch.setattr(_C, "dot_attn_bwd_src", lambda *a, **k: (calls.append(("src", k.get("want_dk"), k.get("want_dv"))), real_src(*a, **k))[1])
    g2 = PG.SG.small_graph(20, 30, 8).to(DEV)
    E = g2.number_of_edges()
    x = [torch.randn(20, 2, 4, device=DEV), torch.randn(30, 2, 4, device=DEV), torch.randn(30, 2, 4, device=DEV), torch.randn(8, 3, device=DEV)]
    ef = torch.randn(E, 3, device=DEV)
    run = lambda leaves: ops.dot_attention_edge(g2, leaves[0], leaves[1], leaves[2], ef, leaves[3]).sum().backward()
    full = [t.clone().requires_grad_() for t in x]
    run(full)
    assert calls == [("dst", True, True), ("src", True, True)]
    g2._csr = None
    for need, seen in (((True, False, False, False), [("dst", True, True)]), ((False, False, False, True), [("dst", False, True)]),
                       ((False, True, False, False), [("dst", False, False), ("src", True, False)]),
                       ((False, False, True, False), [("dst", False, False), ("src", False, True)])):
        calls.clear()
        leaves = [t.clone().requires_grad_(r) for t, r in zip(x, need)]
        run(leaves)
        assert calls == seen, (need, calls)
        if need[0] or need[3]:
            assert g2._csr is None                                    # the CSR is built only when k or v needs a gradient
        i = need.index(True)
        if i in (1, 2):
            assert _same(leaves[i].grad, full[i].grad)
        else:                                                         # (dense products around the sweep: other operands, other roundings)
            assert torch.allclose(leaves[i].grad, full[i].grad, rtol=1e-4, atol=1e-5)


@pytest.mark.gpu
def test_nan_stays_inside_the_destinations_and_heads_that_read_it():
    name, g = _graphs()[6]
    src, dst = EC.positions(g)
    n_src, n_dst, E = g.number_of_src_nodes(), g.number_of_dst_nodes(), src.numel()
    H, D, K = 3, 5, 3
    q, k, v, dout, ef, _, qe, daef = (t.to(DEV) for t in EC.normal_inputs(n_src, n_dst, E, H, D, K, 4))
    clean = _C.dot_attn_edge(g.csc, q, k, v, qe, ef, 0.5)
    pos = E // 2                                                          # one ef row: every head of its destination, nothing else
    ef2 = ef.clone()
    ef2[pos, 1] = float("nan")
    got = _C.dot_attn_edge(g.csc, q, k, v, qe, ef2, 0.5)
    hit = torch.zeros(n_dst, dtype=torch.bool, device=DEV)
    hit[int(dst[pos])] = True
    for a, b in zip(got, clean):
        assert bool(torch.isnan(a[hit]).any()) and _same(a[~hit], b[~hit])
    assert bool(torch.isnan(got[1][hit]).all())                           # lse of every head of that destination
    row = int(dst[0])                                                     # one qe row of one head: that destination's head alone
    qe2 = qe.clone()
    qe2[row, 1, 0] = float("nan")
    got = _C.dot_attn_edge(g.csc, q, k, v, qe2, ef, 0.5)
    mask = torch.zeros(n_dst, H, dtype=torch.bool, device=DEV)
    mask[row, 1] = True
    for a, b in zip(got, clean):
        m = mask if a.dim() == 2 else mask.unsqueeze(-1).expand_as(a)
        assert bool(torch.isnan(a[m]).all()) and _same(a[~m], b[~m])
    dq, dqe, pw, ds = _C.dot_attn_edge_bwd_dst(g.csc, q, k, v, qe2, ef, 0.5, None, 0.0, dout, daef, *clean)
    dq0, dqe0, pw0, ds0 = _C.dot_attn_edge_bwd_dst(g.csc, q, k, v, qe, ef, 0.5, None, 0.0, dout, daef, *clean)
    m3 = mask.unsqueeze(-1)
    assert _same(dq[~m3.expand_as(dq)], dq0[~m3.expand_as(dq)]) and _same(dqe[~m3.expand_as(dqe)], dqe0[~m3.expand_as(dqe)])
    em = mask[dst.to(DEV)]
    assert _same(pw[~em], pw0[~em]) and _same(ds[~em], ds0[~em]) and bool(torch.isnan(ds[em]).all())


# ------------------------------------------------------------------------------------------------ 3. layers, stack, recipe
def _edata(g, K, seed):
    g.edata["feat"] = torch.randn(g.number_of_edges(), K, generator=torch.Generator().manual_seed(seed)).to(DEV)
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("concat", [False, True])
@pytest.mark.parametrize("beta", [False, True])
def test_edge_transformerconv_against_fp64_restatement(concat, beta):
    kw = dict(concat=concat, beta=beta, edge_dim=4)
    g, sub, b = PG._parent(), PG._subgraph(), PG._block()
    ef = lambda x, s: torch.randn(x.number_of_edges(), 4, generator=torch.Generator().manual_seed(s))
    torch.manual_seed(0)
    EC.check_layer(DC.seeded(bnn.EdgeTransformerConv(8, 5, 3, **kw), 0), g, DEV, 8, ef(g, 1))
    assert ops.dot_attn_last_impl == "kernel"
    EC.check_layer(DC.seeded(bnn.EdgeTransformerConv(8, 5, 3, allow_zero_in_degree=True, **kw), 1), sub, DEV, 8, ef(sub, 2), seed=2)
    EC.check_layer(DC.seeded(bnn.EdgeTransformerConv(8, 8, 2, bias=False, allow_zero_in_degree=True, **kw), 2), b, DEV, 8, ef(b, 3), pair=True, seed=3)
    EC.check_layer(DC.seeded(bnn.EdgeTransformerConv(8, 4, 1, allow_zero_in_degree=True, **kw), 3), b, DEV, 8, ef(b, 4), seed=4)
    assert ops.dot_attn_last_impl == "kernel"


@pytest.mark.gpu
def test_edge_unimp_stack_against_fp64_restatement():
    g = _edata(PG._parent(), 4, 0)                                     # (K = 4: the output layer's heads are n_classes = 5 wide, and D >= K)
    torch.manual_seed(3)
    model = bnn.EdgeUniMP(8, 5, 8, 3, 2, F.relu, norm="batch", dropout=0.5, attn_drop=0.1, edge_dim=4)
    EC.check_stack(model, g, g.ndata["feat"].cpu(), DEV)
    assert ops.dot_attn_last_impl == "kernel"
    sub = PG._subgraph()
    EC.check_stack(bnn.EdgeUniMP(8, 5, 8, 2, 2, F.relu, edge_dim=4), sub, sub.ndata["feat"].cpu(), DEV,
                   edge_feats=torch.randn(sub.number_of_edges(), 4, generator=torch.Generator().manual_seed(6)).to(DEV))
    nids = torch.randperm(g.number_of_nodes(), generator=torch.Generator().manual_seed(3))[:600]
    _, _, blocks = next(iter(NodeDataLoader(g, nids, MultiLayerNeighborSampler([5, 7, 9]), batch_size=600, seed=4)))
    EC.check_stack(bnn.EdgeUniMP(8, 5, 8, 3, 2, F.relu, beta=False, edge_dim=4), blocks, blocks[0].srcdata["feat"].cpu(), DEV)
    assert ops.dot_attn_last_impl == "kernel"


@pytest.mark.gpu
def test_build_unimp_edge_full_batch_step():
    wl = workloads.build_unimp_edge("proteins", DEV, scale=0.02)
    before = [p.detach().clone() for p in wl.model.parameters()]
    torch.manual_seed(0)
    loss, pred = wl.step()
    assert np.isfinite(float(loss.detach())) and bool(torch.isfinite(pred).all()) and ops.dot_attn_last_impl == "kernel"
    for name, p in wl.model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    assert all(float(c.lin_edge.weight.grad.abs().max()) > 0 for c in wl.model.convs[1:])
    assert any(not torch.equal(p.detach(), b) for p, b in zip(wl.model.parameters(), before))


@pytest.mark.gpu
def test_build_unimp_edge_sampled_epoch():
    wl = workloads.build_unimp_edge("proteins", DEV, sampled=True, scale=0.02)
    before = [p.detach().clone() for p in wl.model.parameters()]
    torch.manual_seed(0)
    loss = wl.epoch()
    assert np.isfinite(float(torch.as_tensor(loss).detach())) and ops.dot_attn_last_impl == "kernel"
    for name, p in wl.model.named_parameters():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()), name
    assert any(not torch.equal(p.detach(), b) for p, b in zip(wl.model.parameters(), before))
