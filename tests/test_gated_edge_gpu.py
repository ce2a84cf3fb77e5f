"""Gated aggregation with an edge stream on the MI355X: the three sweeps of csrc/spmm_gate_edge.hip against the float64 restatement
(tests/gated_edge_cases.py) - entry for entry in the exact regimes (integer-valued operands, c chosen per position so that every gate is
0.5, 1 or 0), strided and aliased per-edge operands, every optional pointer present and absent, the long-row chunks, repeatability -
and under the derived bounds on seeded normal inputs, the kernel form against the tensor form; `ops.gated_edge_sum` (orders,
want_edge, needed gradients only), `nn.GatedGCNConv` and `nn.GatedGCN` against their float64 restatements under the suite's own criteria
(tests/parity_cases.py), and the steps of `workloads.build_gatedgcn` / `build_gatedgcn_clustered`.

Largest error seen as a fraction of its derived bound (run with -s to print them): README "GatedGCN with an edge stream"."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bot_amd
from bot_amd import _C, ops, workloads
from bot_amd import nn as bnn
from tests import block_cases as BC
from tests import gated_edge_cases as EC
from tests import sage_cases as SG

pytestmark = pytest.mark.gpu
DEV = "cuda"
# 1 the smallest; 3, 5 odd widths, 4-byte lanes; 4 one 16-byte lane; 63, 65 odd widths around a wavefront of 4-byte lanes (65: tiles); 64 a
# group of 16 lanes; 256 a wavefront of 16-byte lanes; 1000 walks tiles of 16-byte lanes
WIDTHS = (1, 3, 4, 5, 63, 64, 65, 256, 1000)
WORST = {}


@functools.lru_cache(maxsize=None)
def _graphs():
    """(name, graph on the device): a one-edge graph, 1 / 63 / 64 / 65 square rows with isolated rows and parallel edges, chunk = 4
    variants (long rows in both directions: the workspace and the combine at small sizes), and a block with n_dst < n_src."""
    out = [("one_edge", bot_amd.Graph(torch.tensor([0]), torch.tensor([0]), 1).to(DEV))]
    out += [(f"square{n}", SG.small_graph(n, n, n).to(DEV)) for n in (1, 63, 64, 65)]
    out.append(("long65", SG.small_graph(65, 65, 70, chunk=4).to(DEV)))
    out.append(("block", SG.small_graph(63, 200, 71).to(DEV)))
    out.append(("longblock", SG.small_graph(64, 130, 72, chunk=4).to(DEV)))
    for i in (5, 7):
        assert out[i][1].csc.n_long > 0 and out[i][1].csr.n_long > 0
    assert out[1][1].csc.n_long == 0
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _hub():
    """A row above the row planner's own long-row threshold at its default chunk, in both directions."""
    from tests.test_subgraph_gpu import _hub_graph
    g = _hub_graph()
    chunk = _C.default_chunk(g.csc.nnz)
    assert int(np.diff(g.csc.indptr.cpu().numpy()).max()) > chunk and int(np.diff(g.csr.indptr.cpu().numpy()).max()) > chunk
    assert g.csc.n_long > 0 and g.csr.n_long > 0
    return g


@functools.lru_cache(maxsize=None)
def _big():
    """About 5 600 edges: a wrong position cannot hide."""
    g = SG.small_graph(1200, 1500, 21).to(DEV)
    assert g.number_of_edges() >= 5000
    return g


def _slab(t, pad, fill=7.0):
    """A device view of the [n, F] tensor `t` whose rows sit in a buffer `pad` floats wider (row pitch F + pad), and the buffer."""
    n, w = t.shape
    buf = torch.full((n, w + pad), fill, dtype=t.dtype, device=DEV)
    buf[:, :w].copy_(t.to(DEV))
    return buf[:, :w], buf


def _out(n, w, pad):
    return _slab(torch.full((n, w), 9.0), pad, 9.0)


def _merged(q, v):
    """q and v as the two column blocks of ONE [n_src, 2F] matrix, the layer's packing."""
    buf = torch.cat((q, v), dim=1).to(DEV)
    Fw = q.shape[1]
    return buf[:, :Fw], buf[:, Fw:]


def _same_bytes(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _eq(got, want):
    return np.array_equal(got.detach().cpu().double().numpy(), want.numpy())


def _untouched(*bufs_w):
    return all(bool((buf[:, w:] == 9.0).all()) for buf, w in bufs_w)


def _check_exact(g, Fw, pad, seed, lim=8, full=True):
    """The three entry points in the exact regimes, entry for entry.  pad > 0: every operand and output with a row pitch of Fw + pad and a
    sentinel behind every output row; pad < 0: q and v as the two blocks of one merged matrix, dq and dv as the blocks of one gradient."""
    src, dst = EC.positions(g)
    n_src, n_dst, E = g.number_of_src_nodes(), g.number_of_dst_nodes(), src.numel()
    csc, csr, pos = g.csc, g.csr, g.csr2csc
    k, q, v, c, a, b, de, s = EC.exact_inputs(src, dst, n_src, n_dst, Fw, seed, lim)
    merged = pad < 0
    pad = max(pad, 0)
    qd, vd = _merged(q, v) if merged else (_slab(q, pad)[0], _slab(v, pad)[0])
    kd, cd, ad, bd, ded = (_slab(t, pad)[0] for t in (k, c, a, b, de))
    deg = np.diff(csc.indptr.cpu().numpy()).astype(np.float32).reshape(-1, 1)
    ref = EC.exact_reference(src, dst, n_src, n_dst, s, v, a, None, de)
    # ---- forward, plain: out, e; e absent; two calls
    (o_v, o_b), (e_v, e_b) = _out(n_dst, Fw, pad), _out(E, Fw, pad)
    out, den, e = _C.spmm_gate_edge(csc, kd, qd, vd, cd, out=o_v, e=e_v)
    assert den is None and (E == 0 or "spmm_gate_edge_kernel<0," in _C._lib.bot_last_kernel().decode())
    assert _eq(out, ref["num"]) and _eq(e, ref["e"]) and _eq(e, (k[dst] + q[src] + c).double()), (Fw, pad)
    assert bool((out[torch.from_numpy(deg[:, 0] == 0).to(DEV)] == 0).all()) and _untouched((o_b, Fw), (e_b, Fw))
    out2, _, none = _C.spmm_gate_edge(csc, kd, qd, vd, cd, want_e=False)
    out3, _, e3 = _C.spmm_gate_edge(csc, kd, qd, vd, cd)
    assert none is None and _same_bytes(out2, out) and _same_bytes(out3, out) and _same_bytes(e3, e)
    alias_v, alias_b = _slab(c, pad, 9.0)                                     # e aliasing c: the bytes of the separate-buffer call
    out4, _, e4 = _C.spmm_gate_edge(csc, kd, qd, vd, alias_v, e=alias_v)
    assert e4.data_ptr() == alias_v.data_ptr() and _same_bytes(out4, out) and _same_bytes(alias_v, e) and _untouched((alias_b, Fw))
    # ---- forward, normalised: float32(num) / (float32(den) + eps) bit for bit, den exact
    (d_v, d_b) = _out(n_dst, Fw, pad)
    for eps in (1e-6, 0.5):
        on, dn, en = _C.spmm_gate_edge(csc, kd, qd, vd, cd, normalize=True, eps=eps, den=d_v)
        assert E == 0 or "spmm_gate_edge_kernel<1," in _C._lib.bot_last_kernel().decode()
        num32, den32 = ref["num"].numpy().astype(np.float32), ref["den"].numpy().astype(np.float32)
        want_n = np.where(deg > 0, num32 / (den32 + np.float32(eps)), np.float32(0)).astype(np.float32)
        assert np.array_equal(on.cpu().numpy().view(np.int32), want_n.view(np.int32)), (Fw, pad, eps)
        assert _eq(dn, ref["den"]) and _same_bytes(en, e) and _untouched((d_b, Fw))
    # ---- backward over the CSC: with and without b, de, ds, dk; ds aliasing de
    for bb, bdev in ((None, None), (b, bd)) if full else ((b, bd),):
        for dd, ddev in ((de, ded), (None, None)) if full else ((de, ded),):
            r = EC.exact_reference(src, dst, n_src, n_dst, s, v, a, bb, dd)
            (s_v, s_b), (k_v, k_b) = _out(E, Fw, pad), _out(n_dst, Fw, pad)
            ds, dk = _C.spmm_gate_edge_bwd(csc, vd, e, ad, bdev, ddev, out_ds=s_v, out_dk=k_v)
            assert E == 0 or f"spmm_gate_edge_bwd_kernel<{int(bb is not None)}," in _C._lib.bot_last_kernel().decode()
            assert _eq(ds, r["ds"]) and _eq(dk, r["dk"]) and _untouched((s_b, Fw), (k_b, Fw)), (Fw, pad, bb is None, dd is None)
            ds2, dk2 = _C.spmm_gate_edge_bwd(csc, vd, e, ad, bdev, ddev)                       # the same bytes on a second call
            only_s, n1 = _C.spmm_gate_edge_bwd(csc, vd, e, ad, bdev, ddev, want_dk=False)
            n2, only_k = _C.spmm_gate_edge_bwd(csc, vd, e, ad, bdev, ddev, want_ds=False)
            assert n1 is None and n2 is None and all(_same_bytes(x, y) for x, y in ((ds2, ds), (dk2, dk), (only_s, ds), (only_k, dk)))
            if dd is not None:
                al_v, al_b = _slab(de, pad, 9.0)
                ds5, dk5 = _C.spmm_gate_edge_bwd(csc, vd, e, ad, bdev, al_v, out_ds=al_v)
                assert _same_bytes(al_v, ds) and _same_bytes(dk5, dk) and _untouched((al_b, Fw))
            # ---- backward over the CSR, from this ds: both outputs, each alone, one merged gradient
            (q_v, q_b), (v_v, v_b) = _out(n_src, Fw, pad), _out(n_src, Fw, pad)
            dq, dv = _C.spmm_gate_edge_bwd_src(csr, pos, e, ds, ad, out_dq=q_v, out_dv=v_v)
            assert E == 0 or "spmm_gate_edge_bwd_src_kernel<" in _C._lib.bot_last_kernel().decode()
            assert _eq(dq, r["dq"]) and _eq(dv, r["dv"]) and _untouched((q_b, Fw), (v_b, Fw)), (Fw, pad)
            only_q, n3 = _C.spmm_gate_edge_bwd_src(csr, pos, None, ds, None, want_dv=False)    # the other output's operands are not needed
            n4, only_v = _C.spmm_gate_edge_bwd_src(csr, pos, e, None, ad, want_dq=False)
            assert n3 is None and n4 is None and _same_bytes(only_q, dq) and _same_bytes(only_v, dv)
            if merged:
                both = torch.full((n_src, 2 * Fw), 9.0, device=DEV)
                _C.spmm_gate_edge_bwd_src(csr, pos, e, ds, ad, out_dq=both[:, :Fw], out_dv=both[:, Fw:])
                assert _same_bytes(both[:, :Fw], dq) and _same_bytes(both[:, Fw:], dv)
    nt = _C.spmm_gate_edge(csc, kd, qd, vd, cd, stream_nt=True)                                 # non-temporal stream rows: the same bytes
    assert _same_bytes(nt[0], out) and _same_bytes(nt[2], e)
    ds_t, dk_t = _C.spmm_gate_edge_bwd(csc, vd, e, ad, bd, ded)
    ds_nt, dk_nt = _C.spmm_gate_edge_bwd(csc, vd, e, ad, bd, ded, stream_nt=True)
    assert _same_bytes(ds_nt, ds_t) and _same_bytes(dk_nt, dk_t)


# ------------------------------------------------------------------------------------------------ 1. exact
@pytest.mark.parametrize("Fw", WIDTHS)
def test_exact_regimes_entry_for_entry(Fw):
    for i, (name, g) in enumerate(_graphs()):
        for pad in (0, 3, 4, -1):
            _check_exact(g, Fw, pad, seed=17 * i + Fw + pad)


def test_exact_regimes_on_the_hub_graph():
    """Rows above the long-row threshold in both directions: the chunks store e and ds at their own positions.  The ranges are shrunk so
    that every sum's absolute terms stay below 2^22."""
    _check_exact(_hub(), 5, 0, seed=3, lim=2, full=False)           # (b and de present; their absence: the small graphs)


# ------------------------------------------------------------------------------------------------ 2. rounded, and the two forms
def _check_kernels_with_b(g, Fw, seed):
    """The sweeps with a given (a, b, de) - the normalised instances - against float64 under the derived bounds."""
    src, dst = EC.positions(g)
    n_src, n_dst = g.number_of_src_nodes(), g.number_of_dst_nodes()
    k, q, v, c, a, b, de = EC.normal_inputs(n_src, n_dst, src.numel(), Fw, seed)
    d = [t.double() for t in (k, q, v, c, a, b, de)]
    fwd = EC.forward64(src, dst, *d[:4], True, 1e-6)
    want = EC.backward64(src, dst, fwd["e"], d[2], d[4], d[5], d[6])
    bnd = EC.bounds(src, dst, *d[:4], d[4], d[5], d[6])
    kd, cd, ad, bd, ded = (t.to(DEV) for t in (k, c, a, b, de))
    qd, vd = _merged(q, v)
    out, den, e = _C.spmm_gate_edge(g.csc, kd, qd, vd, cd, normalize=True, eps=1e-6)
    ds, dk = _C.spmm_gate_edge_bwd(g.csc, vd, e, ad, bd, ded)
    dq, dv = _C.spmm_gate_edge_bwd_src(g.csr, g.csr2csc, e, ds, ad)
    for name, x, y in (("e", e, fwd["e"]), ("den", den, fwd["den"]), ("out", out, fwd["out"]), ("ds", ds, want["ds"]), ("dk", dk, want["dk"]),
                       ("dq", dq, want["dq"]), ("dv", dv, want["dv"])):
        err = (x.cpu().double() - y).abs()
        frac = EC._record(WORST, "kernel with b " + name, err, bnd[name])
        assert bool((err <= bnd[name]).all()), (name, Fw, frac)


@pytest.mark.parametrize("Fw", WIDTHS)
def test_kernel_and_tensor_forms_against_fp64_under_derived_bounds(Fw):
    for i in (4, 5, 6, 7):
        name, g = _graphs()[i]
        for normalize in (False, True):
            got_k = EC.check_op(g, DEV, Fw, seed=i + Fw, impl="kernel", normalize=normalize, worst=WORST)
            got_t = EC.check_op(g, DEV, Fw, seed=i + Fw, impl="tensor", normalize=normalize, worst=WORST)
            assert torch.allclose(got_k[0], got_t[0], rtol=1e-4, atol=1e-5) and torch.allclose(got_k[1], got_t[1], rtol=1e-5, atol=1e-5)
        _check_kernels_with_b(g, Fw, seed=i + 2 * Fw)
    print("largest error / bound so far:", {k: round(v, 4) for k, v in sorted(WORST.items())})
    assert all(v <= 1.0 for v in WORST.values())


@pytest.mark.parametrize("Fw", [5, 128])
def test_normal_inputs_on_5000_edges_against_fp64_under_derived_bounds(Fw):
    for normalize in (False, True):
        for impl in ("kernel", "tensor"):
            EC.check_op(_big(), DEV, Fw, seed=Fw, impl=impl, normalize=normalize, worst=WORST)
            EC.check_op(_big(), DEV, Fw, seed=Fw + 1, impl=impl, normalize=normalize, worst=WORST, with_de=False)
    _check_kernels_with_b(_big(), Fw, seed=Fw + 2)
    print("largest error / bound so far:", {k: round(v, 4) for k, v in sorted(WORST.items())})
    assert all(v <= 1.0 for v in WORST.values())


def test_hub_graph_against_fp64_under_derived_bounds():
    """Rows above the long-row threshold in both directions: the outputs and the four gradients.  (The normalised instances' long
    rows: the chunk = 4 graphs above.)"""
    EC.check_op(_hub(), DEV, 5, seed=2, impl="kernel", normalize=False, worst=WORST)
    print("largest error / bound so far:", {k: round(v, 4) for k, v in sorted(WORST.items())})
    assert all(v <= 1.0 for v in WORST.values())


# ------------------------------------------------------------------------------------------------ 3. the op
def test_eid_order_against_csc_order_on_a_shuffled_edge_list():
    g = _graphs()[6][1]                                   # built from a shuffled edge list: edge ids are not positions
    perm = g.csc.eid.long()
    assert not torch.equal(perm, torch.arange(perm.numel(), device=DEV))
    k, q, v, c, dout, _, de = (t.to(DEV) for t in EC.normal_inputs(200, 63, perm.numel(), 6, 2))
    leaves = [t.clone().requires_grad_() for t in (k, q, v, c)]
    out, e = ops.gated_edge_sum(g, *leaves, order="csc", impl="kernel")
    torch.autograd.backward([out, e], [dout, de])
    c_eid = torch.empty_like(c).index_copy_(0, perm, c).requires_grad_()
    leaves2 = [t.clone().requires_grad_() for t in (k, q, v)]
    out2, e2 = ops.gated_edge_sum(g, *leaves2, c_eid, impl="kernel")                 # order="eid" is the default
    torch.autograd.backward([out2, e2], [dout, torch.empty_like(de).index_copy_(0, perm, de)])
    assert _same_bytes(out2, out) and _same_bytes(e2[perm], e) and _same_bytes(c_eid.grad[perm], leaves[3].grad)
    assert all(_same_bytes(x.grad, y.grad) for x, y in zip(leaves2, leaves))
    sub = _subgraph()                                                                # a Subgraph's edge ids ARE its positions
    assert ops._csc_edge_rows(sub) is None


def test_want_edge_false_and_nothing_per_edge_under_no_grad(monkeypatch):
    g = _graphs()[6][1]
    E = g.number_of_edges()
    k, q, v, c = (t.to(DEV) for t in EC.normal_inputs(200, 63, E, 6, 3)[:4])
    seen = []
    real = _C.spmm_gate_edge
    monkeypatch.setattr(_C, "spmm_gate_edge", lambda *a, **kw: (seen.append(kw["want_e"]), real(*a, **kw))[1])
    full, e = ops.gated_edge_sum(g, k, q, v, c, order="csc", impl="kernel")
    with torch.no_grad():
        out, none = ops.gated_edge_sum(g, k, q, v, c, order="csc", want_edge=False, impl="kernel")
    assert none is None and seen == [True, False] and _same_bytes(out, full)         # e = NULL: nothing per edge is written
    leaves = [t.clone().requires_grad_() for t in (k, q, v, c)]
    out, none = ops.gated_edge_sum(g, *leaves, order="csc", want_edge=False, impl="kernel")   # with gradients e is kept for the backward
    assert none is None and seen[-1] is True
    out.sum().backward()
    ref = [t.clone().requires_grad_() for t in (k, q, v, c)]
    ops.gated_edge_sum(g, *ref, order="csc", impl="kernel")[0].sum().backward()
    assert all(_same_bytes(x.grad, y.grad) for x, y in zip(leaves, ref))


def test_needed_gradients_only(monkeypatch):
    calls = []
    real_csc, real_src = _C.spmm_gate_edge_bwd, _C.spmm_gate_edge_bwd_src
    monkeypatch.setattr(_C, "spmm_gate_edge_bwd", lambda *a, **k: (calls.append(("csc", k["want_ds"], k["want_dk"])), real_csc(*a, **k))[1])
    monkeypatch.setattr(_C, "spmm_gate_edge_bwd_src", lambda *a, **k: (calls.append(("src", k["want_dq"], k["want_dv"])), real_src(*a, **k))[1])
    full = None
    for normalize in (False, True):
        for need, seen in (((True, True, True, True), [("csc", True, True), ("src", True, True)]),
                           ((True, False, False, False), [("csc", False, True)]), ((False, False, False, True), [("csc", True, False)]),
                           ((True, False, False, True), [("csc", True, True)]), ((False, True, False, False), [("csc", True, False), ("src", True, False)]),
                           ((False, False, True, False), [("src", False, True)])):
            g2 = SG.small_graph(20, 30, 8).to(DEV)
            x = [t.to(DEV) for t in EC.normal_inputs(30, 20, g2.number_of_edges(), 8, 1)[:4]]
            calls.clear()
            leaves = [t.clone().requires_grad_(r) for t, r in zip(x, need)]
            out, e = ops.gated_edge_sum(g2, *leaves, normalize=normalize, order="csc", impl="kernel")
            (out.sum() + (e * e).sum()).backward()
            assert calls == seen, (need, calls)
            src_side = need[1] or need[2]
            assert (g2._csr is None) == (not src_side)                               # the CSR is built only for dq or dv
            grads = [t.grad for t in leaves]
            if all(need):
                full = grads
            else:                                                                    # a subset gives the bytes of the full backward
                assert all(a is None or _same_bytes(a, b) for a, b in zip(grads, full))


def test_impl_selection_is_read_at_call_time(monkeypatch):
    g = _graphs()[6][1]
    monkeypatch.setenv("BOT_GATE_EDGE", "tensor")
    calls = []
    real = _C.spmm_gate_edge
    monkeypatch.setattr(_C, "spmm_gate_edge", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    EC.check_op(g, DEV, 5, seed=2)
    assert calls == []
    EC.check_op(g, DEV, 5, seed=2, impl="kernel")                                    # the argument wins over the variable
    assert calls == [1]
    monkeypatch.delenv("BOT_GATE_EDGE")
    EC.check_op(g, DEV, 5, seed=2)
    assert len(calls) == (2 if ops.gate_edge_default_impl == "kernel" else 1)


# ------------------------------------------------------------------------------------------------ 4. layer, stack, recipes
@functools.lru_cache(maxsize=None)
def _parent():
    g = BC.parent_graph(DEV, n=3000, e_raw=20000, fin=7)
    g.edata["feat"] = torch.randn(g.number_of_edges(), 3, generator=torch.Generator().manual_seed(8)).to(DEV)
    return g


@functools.lru_cache(maxsize=None)
def _subgraph():
    g = _parent()
    nodes = torch.randperm(g.number_of_nodes(), generator=torch.Generator().manual_seed(4))[:1200].sort().values
    return g.subgraph(nodes.to(DEV))


@functools.lru_cache(maxsize=None)
def _block():
    from bot_amd.sampling import sample_block
    g = _parent()
    seeds = torch.randperm(g.number_of_nodes(), generator=torch.Generator().manual_seed(2))[:500].to(DEV, torch.int32)
    b = sample_block(g, seeds, 5, 77)
    assert b.number_of_src_nodes() > b.number_of_dst_nodes()
    return b


@pytest.mark.parametrize("batch_norm", [False, True])
@pytest.mark.parametrize("residual", [False, True])
def test_gatedgcnconv_against_fp64_restatement(batch_norm, residual):
    kw = dict(batch_norm=batch_norm, residual=residual)
    EC.check_conv(_parent(), DEV, 8, 8, 8, **kw)
    EC.check_conv(_parent(), DEV, 8, 3, 64, seed=1, order="csc", activation=F.elu, **kw)
    EC.check_conv(_parent(), DEV, 6, 6, 6, seed=2, order="csc", edge_out=False, **kw)
    EC.check_conv(_subgraph(), DEV, 8, 4, 6, seed=3, **kw)
    EC.check_conv(_block(), DEV, 8, 8, 8, seed=4, **kw)


def test_merged_projection_reaches_the_sweeps_as_one_matrix():
    from bot_amd import gemm
    g = _parent()
    seen = []
    real = ops.gated_edge_sum
    conv = EC.make_conv(128, 128, 128, 5).to(DEV)
    x, ef = torch.randn(g.number_of_nodes(), 128, device=DEV), torch.randn(g.number_of_edges(), 128, device=DEV)
    old = gemm.MIN_ROWS
    gemm.MIN_ROWS = 1024
    try:
        ops.gated_edge_sum = lambda gr, k, q, v, c, **kw: (seen.append((q, v)), real(gr, k, q, v, c, **kw))[1]
        h, e = conv(g, x, ef)
    finally:
        ops.gated_edge_sum, gemm.MIN_ROWS = real, old
    q, v = seen[0]
    assert q.shape == (g.number_of_nodes(), 128) and q.stride() == (256, 1) and v.stride() == (256, 1)
    assert v.data_ptr() == q.data_ptr() + 128 * 4 and bool(torch.isfinite(h).all()) and bool(torch.isfinite(e).all())
    EC.check_conv(g, DEV, 128, 128, 128, seed=5)


def test_gatedgcn_stack_against_fp64_restatement():
    torch.manual_seed(3)
    EC.check_stack(bnn.GatedGCN(7, 3, 5, 6, 3), _parent(), DEV)
    torch.manual_seed(4)
    EC.check_stack(bnn.GatedGCN(7, 3, 5, 16, 3, residual=False), _subgraph(), DEV)
    with pytest.raises(ValueError, match="each block has its own edges"):
        bnn.GatedGCN(7, 3, 5, 6, 2).to(DEV)([_block(), _block()])


def _finite_grads(model):
    skip = f"convs.{model.n_layers - 1}.bn_edge"                                     # the last layer has no edge output
    return all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for n, p in model.named_parameters() if not n.startswith(skip))


@pytest.mark.parametrize("name", ["arxiv", "proteins"])
def test_build_gatedgcn_full_batch_step(name):
    wl = workloads.build_gatedgcn(name, DEV, scale=0.02 if name == "arxiv" else 0.0005)
    torch.manual_seed(0)
    losses = [float(wl.step()[0].detach()) for _ in range(3)]
    assert all(np.isfinite(v) for v in losses), losses
    assert _finite_grads(wl.model)


def test_build_gatedgcn_clustered_batch():
    wl = workloads.build_gatedgcn_clustered("arxiv", DEV, scale=0.02, n_parts=4)
    torch.manual_seed(0)
    res = wl.step(next(iter(wl.loader)))
    assert res is not None and np.isfinite(float(res[0].detach())) and _finite_grads(wl.model)
    with pytest.raises(ValueError, match="build_gatedgcn_clustered"):
        workloads.build_gatedgcn("proteins", DEV)


# ------------------------------------------------------------------------------------------------ 5. errors
def test_error_paths():
    name, g = _graphs()[4]
    n, E = g.number_of_nodes(), g.number_of_edges()
    x, c = torch.randn(n, 8, device=DEV), torch.randn(E, 8, device=DEV)
    assert ops.gated_edge_sum(g, x, x, x, c)[1].shape == (E, 8)
    from bot_amd.errors import DGLError
    for bad, text in (((x[:-1], x, x, c), f"({n - 1}, 8)"), ((x, x, x, c[:, :4]), f"({E}, 4)"), ((x, x, x, c.cpu()), "cpu"),
                      ((x, x, x.double(), c), "float64")):
        with pytest.raises(DGLError) as err:
            ops.gated_edge_sum(g, *bad)
        assert text in str(err.value)
    with pytest.raises(_C.BotKernelError, match="unit inner stride"):
        _C.spmm_gate_edge(g.csc, x, x, x, c.t().contiguous().t())
    with pytest.raises(_C.BotKernelError, match="alias"):
        _C.spmm_gate_edge(g.csc, x, x, x, c, out=x)
    part = BC.parent_graph(DEV, n=200, e_raw=1500, seed=7)
    part.halo = object()                                                              # a partition's block carries a halo plan
    with pytest.raises(ValueError, match="partition"):
        ops.gated_edge_sum(part, *(torch.randn(200, 4, device=DEV) for _ in range(3)), torch.randn(part.number_of_edges(), 4, device=DEV))
