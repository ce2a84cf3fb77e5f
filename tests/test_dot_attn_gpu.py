"""Dot-product attention on the MI355X: the three sweeps of csrc/dot_attn.hip against the float64 restatement (tests/dot_attn_cases.py)
- entry for entry in the two exact regimes (uniform weights, one-hot weights) and under bounds derived from the lengths on seeded normal
inputs - the kernel form against the tensor form, `nn.DotGatConv`, `nn.TransformerConv` and `nn.UniMP` against their float64
restatements under the suite's own criteria (tests/parity_cases.py), and the steps of `workloads.build_unimp`.

One-hot regime, gradients: the backward's weight is exp(s - lse).  Where a row has ONE maximal in-edge lse = s and the weight is exactly
1: those entries are compared entry for entry with the ideal sums (ds is 0 there, so dq and dk are exact zeros and dv an exact sum).
Where it has m > 1 of them (parallel edges; the one-row graph is such a row) lse = s + log m is rounded at the size of s (up to 2^31
here), so exp(s - lse) is 1 / m only to within that rounding and NO kernel that reads a float32 lse can give the ideal sums there.
EVERY entry, those rows included, is therefore also held to the sums the contract itself defines from the float32 lse the kernel
returned (held to 3 U |lse|) and its float32 out (bit for bit): with a = exp(s - lse32) in float64 - s and s - lse are exact float32
here - the only errors left are smx_exp's measured 1.278e-07 (margin 2) and the sums' own roundings, a few 1e-7 of the absolute terms
whatever the size of the logits (tests/dot_attn_cases.onehot_backward_from_lse).  With a keep mask the tie rows' ds is not 0, so dq
and dk get a non-trivial check there on every graph; the normal-input test runs all seven graphs too.

Largest error seen as a fraction of its derived bound (run with -s to print them), kernel form: out 0.040, dq 0.026, dk 0.023, dv
0.061, dk + dv (shared) 0.063; tensor form: out 0.040, dq 0.031, dk 0.026, dv 0.061, dk + dv 0.029; one-hot regime against the sums
from the returned lse: p 0.080, ds 0.064, dq 0.016, dk 0.014, dv 0.111, dk + dv 0.087 (README "Dot-product attention")."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bot_amd import _C, ops, workloads
from bot_amd import nn as bnn
from bot_amd.sampling import MultiLayerNeighborSampler, NodeDataLoader, sample_block
from tests import block_cases as BC
from tests import dot_attn_cases as DC
from tests import gatv2_cases as GC
from tests import sage_cases as SG

DEV = "cuda"
# (1, 1) the smallest; (1, 3) odd width, 4-byte lanes; (3, 5) heads that end inside a group at odd lanes; (2, 64) / (8, 32) heads that
# are whole spans of lanes; (4, 65) heads straddling 64-lane chunks; (3, 250) the workload's (one tile of six chunks; with an odd row
# stride three tiles of one head); (8, 250) several head tiles
EXACT_PAIRS = ((1, 1), (1, 3), (3, 5), (2, 64), (8, 32), (4, 65), (3, 250), (8, 250))
WIDE = (1, 1600)          # one head wider than a tile: the entry point refuses, the op runs the tensor form
WORST = {}
U = DC.U


def graph_specs():
    """(name, builder of the CPU graph): 1 / 63 / 64 / 65 square rows with isolated rows and parallel edges, chunk = 4 variants (long
    rows: the workspace and both combines at small sizes), and a block and a long block with n_src > n_dst."""
    out = [(f"square{n}", functools.partial(SG.small_graph, n, n, n)) for n in (1, 63, 64, 65)]
    out.append(("long65", functools.partial(SG.small_graph, 65, 65, 70, chunk=4)))
    out.append(("block", functools.partial(SG.small_graph, 63, 200, 71)))
    out.append(("longblock", functools.partial(SG.small_graph, 64, 130, 72, chunk=4)))
    return tuple(out)


def exact_seed(i, H, D):
    return 17 * i + H + D


@functools.lru_cache(maxsize=None)
def _graphs():
    out = tuple((name, make().to(DEV)) for name, make in graph_specs())
    for i in (4, 6):
        assert out[i][1].csc.n_long > 0 and out[i][1].csr.n_long > 0
    assert out[0][1].csc.n_long == 0
    return out


@functools.lru_cache(maxsize=None)
def _hub():
    from tests.test_subgraph_gpu import _hub_graph
    g = _hub_graph()
    assert int(np.diff(g.csc.indptr.cpu().numpy()).max()) > 2048 and g.csc.n_long > 0 and g.csr.n_long > 0
    return g


def _slab(t, pad, fill=7.0):
    """A device view of the [n, ..] tensor `t` whose rows sit in a buffer `pad` floats wider (row stride width + pad)."""
    n, w = t.shape[0], int(np.prod(t.shape[1:]))
    buf = torch.full((n, w + pad), fill, dtype=t.dtype, device=DEV)
    buf[:, :w].copy_(t.reshape(n, w).to(DEV))
    return buf[:, :w].view(t.shape), buf


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _held(got, want, exact, bound, what):
    """Entry for entry where `exact` (a mask, or None), within `bound` (or None) everywhere."""
    err = (got.detach().cpu().double() - want).abs()
    if exact is not None:
        ex = exact.view(exact.shape + (1,) * (err.dim() - exact.dim())).expand_as(err)
        assert bool((err[ex] == 0).all()), (what, "exact entries", float(err[ex].max()))
    if bound is not None:
        assert bool((err <= bound).all()), (what, float((err / bound.clamp(min=1e-300)).max()))


def _run_sweeps(g, q, k, v, dout, scale, keep, p, pad, shared):
    """The three entry points on (possibly strided) operands and outputs -> a dict of results; checks the instances that ran, that two
    calls give the same bytes, that each gradient alone gives the same bytes, and that nothing is written beyond a strided row."""
    n_src, n_dst, E = g.number_of_src_nodes(), g.number_of_dst_nodes(), g.number_of_edges()
    H, D = q.shape[1], q.shape[2]
    csc, csr = g.csc, g.csr
    qd, kd, dd = _slab(q, pad)[0], _slab(k, pad)[0], _slab(dout, pad)[0]
    vd = kd if shared else _slab(v, pad)[0]
    bits = None if keep is None else ops.pack_keep(keep.to(DEV))
    nine = lambda *shape: _slab(torch.full(shape, 9.0), pad, 9.0)
    (o_out, o_buf), (l_out, l_buf) = nine(n_dst, H, D), nine(n_dst, H)
    out, lse = _C.dot_attn(csc, qd, kd, vd, scale, bits, p, out=o_out if pad else None, lse=l_out if pad else None)
    assert f"dot_attn_kernel<{int(shared)}," in _C._lib.bot_last_kernel().decode()
    out2, lse2 = _C.dot_attn(csc, qd, kd, vd, scale, bits, p)
    assert _same(out2, out) and _same(lse2, lse)
    if keep is None:                                                            # keep = all ones and keep = NULL: the same bytes
        ones = torch.full((E,), -1, dtype=torch.int32, device=DEV)
        out3, lse3 = _C.dot_attn(csc, qd, kd, vd, scale, ones, 0.0)
        assert _same(out3, out) and _same(lse3, lse)
    outc, lsec = out, lse                                                       # strided when pad: the backward reads them at ldo, ldl
    dq_out, dq_buf = nine(n_dst, H, D)
    dq, pw, ds = _C.dot_attn_bwd_dst(csc, qd, kd, vd, scale, bits, p, dd, outc, lsec, dq=dq_out if pad else None)
    assert f"dot_attn_bwd_dst_kernel<{int(shared)}," in _C._lib.bot_last_kernel().decode()
    dq2, pw2, ds2 = _C.dot_attn_bwd_dst(csc, qd, kd, vd, scale, bits, p, dd, outc, lsec)
    none, pw3, ds3 = _C.dot_attn_bwd_dst(csc, qd, kd, vd, scale, bits, p, dd, outc, lsec, want_dq=False)
    assert none is None and _same(dq2, dq) and all(_same(a, pw) for a in (pw2, pw3)) and all(_same(a, ds) for a in (ds2, ds3))
    (k_out, k_buf), (v_out, v_buf) = nine(n_src, H, D), nine(n_src, H, D)
    res = dict(out=out, lse=lse, dq=dq, p=pw, ds=ds)
    if shared:
        dkv, same = _C.dot_attn_bwd_src(csr, g.csr2csc, qd, dd, pw, ds, scale, shared=True, dk=k_out if pad else None)
        assert same is dkv and _same(_C.dot_attn_bwd_src(csr, g.csr2csc, qd, dd, pw, ds, scale, shared=True)[0], dkv)
        res["dkv"] = dkv
    else:
        dk, dv = _C.dot_attn_bwd_src(csr, g.csr2csc, qd, dd, pw, ds, scale, dk=k_out if pad else None, dv=v_out if pad else None)
        dk2, dv2 = _C.dot_attn_bwd_src(csr, g.csr2csc, qd, dd, pw, ds, scale)
        dk3, n1 = _C.dot_attn_bwd_src(csr, g.csr2csc, qd, dd, pw, ds, scale, want_dv=False)
        n2, dv3 = _C.dot_attn_bwd_src(csr, g.csr2csc, qd, dd, pw, ds, scale, want_dk=False)
        assert n1 is None and n2 is None and all(_same(a, dk) for a in (dk2, dk3)) and all(_same(a, dv) for a in (dv2, dv3))
        res.update(dk=dk, dv=dv)
    assert "dot_attn_bwd_src_kernel" in _C._lib.bot_last_kernel().decode()
    if pad:                                                                     # nothing is written beyond a strided row
        w = H * D
        assert bool((o_buf[:, w:] == 9.0).all()) and bool((l_buf[:, H:] == 9.0).all()) and bool((dq_buf[:, w:] == 9.0).all())
        assert bool((k_buf[:, w:] == 9.0).all()) and (shared or bool((v_buf[:, w:] == 9.0).all()))
    return res


def _check_uniform(g, H, D, seed, pad, p=0.0, lim=8):
    """Exact regime A: q = 0.  out = c * float32(sum of the kept v) / float32(deg) bit for bit, lse = log(deg) to the rounding of one
    logarithm: OCML's logf is within one ulp (2 U |lse|), the float64 reference's own conversion another U |lse|."""
    (q, k, v, dout), src, dst = DC.uniform_inputs(g, H, D, seed, lim)
    n_dst, E = g.number_of_dst_nodes(), src.numel()
    keep = DC.draw_keep(E, H, p, seed + 1) if p > 0 else None
    res = _run_sweeps(g, q, k, v, dout, D ** -0.5, keep, p, pad, False)
    w = v.double()[src] if keep is None else v.double()[src] * keep.double().unsqueeze(-1)
    tot = torch.zeros(n_dst, H, D, dtype=torch.float64).index_add_(0, dst, w)
    deg = GC.degree_of(dst, n_dst).view(-1, 1, 1)
    want = (1.0 / (1.0 - p)) * (tot.float() / deg.clamp(min=1).float())        # p is 0 or 0.5: the factor is exact
    assert torch.equal(res["out"].cpu(), want), (H, D, pad, p)
    lse = torch.log(deg.clamp(min=1)).view(-1, 1).expand(-1, H)
    assert bool(((res["lse"].cpu().double() - lse).abs() <= 3 * U * lse.abs()).all())


def _check_onehot(g, H, D, seed, pad, shared=False, p=0.0, lim=None):
    """Exact regime B: see tests/dot_attn_cases.onehot_inputs and the module docstring."""
    E = g.number_of_edges()
    n_src, n_dst = g.number_of_src_nodes(), g.number_of_dst_nodes()
    keep = DC.draw_keep(E, H, p, seed + 1) if p > 0 else None
    c = 1.0 / (1.0 - p)
    case = DC.onehot_inputs(g, H, D, seed, lim=lim, shared=shared, keep=keep, c=c)
    fwd, bwd, src, dst = case["fwd"], case["bwd"], case["src"], case["dst"]
    res = _run_sweeps(g, case["q"], case["k"], case["v"], case["dout"], case["scale"], keep, p, pad, shared)
    assert torch.equal(res["out"].cpu(), case["out32"]), (H, D, pad, shared, p)
    assert bool(((res["lse"].cpu().double() - fwd["lse"]).abs() <= 3 * U * fwd["lse"].abs()).all())
    one_dst, one_src = DC.exact_entries(case, n_src)
    want, bb = DC.onehot_backward_from_lse(case, res["lse"].cpu(), D, c, keep)      # every entry, tie rows included: a = exp(s - lse32)
    got = dict(dq=res["dq"], p=res["p"], ds=res["ds"])
    ideal = dict(dq=bwd["dq"], p=bwd["p"], ds=bwd["ds"])
    exact = dict(dq=one_dst, p=one_dst[dst], ds=one_dst[dst])
    if shared:
        got["dkv"], ideal["dkv"], exact["dkv"] = res["dkv"], bwd["dk"] + bwd["dv"], one_src
        want["dkv"] = want["dk"] + want["dv"]
    else:
        got.update(dk=res["dk"], dv=res["dv"]), ideal.update(dk=bwd["dk"], dv=bwd["dv"]), exact.update(dk=one_src, dv=one_src)
    for n in got:
        _held(got[n], ideal[n], exact[n], None, n)                   # one maximal in-edge: the ideal sums, entry for entry
        _held(got[n], want[n], None, bb[n], n)                       # everywhere: the contract's sums from the float32 lse
        if got[n].numel():
            WORST["onehot " + n] = max(WORST.get("onehot " + n, 0.0), float(((got[n].cpu().double() - want[n]).abs() / bb[n].clamp(min=1e-300)).max()))


# ------------------------------------------------------------------------------------------------ 1. exact
@pytest.mark.gpu
@pytest.mark.parametrize("H,D", EXACT_PAIRS)
def test_uniform_weights_are_exact(H, D):
    for i, (name, g) in enumerate(_graphs()):
        for pad, p in ((0, 0.0), (3, 0.0), (4, 0.5)):
            _check_uniform(g, H, D, exact_seed(i, H, D), pad, p)


@pytest.mark.gpu
@pytest.mark.parametrize("H,D", EXACT_PAIRS)
def test_onehot_weights_are_exact(H, D):
    for i, (name, g) in enumerate(_graphs()):
        for pad, shared, p in ((0, False, 0.0), (3, False, 0.0), (4, True, 0.0), (0, True, 0.0), (0, False, 0.5)):
            _check_onehot(g, H, D, exact_seed(i, H, D), pad, shared, p)


@pytest.mark.gpu
def test_exact_regimes_on_the_hub_graph():
    """Rows above 2 048 in-edges at the default chunk; the ranges are shrunk so that every logit stays an exact integer."""
    g = _hub()
    _check_uniform(g, 2, 4, 3, 0, lim=2)
    _check_onehot(g, 2, 4, 3, 0, lim=1)


# ------------------------------------------------------------------------------------------------ 2. rounded, and the two forms
@pytest.mark.gpu
@pytest.mark.parametrize("H,D", EXACT_PAIRS)
def test_kernel_and_tensor_forms_against_fp64_under_derived_bounds(H, D):
    for i, (name, g) in enumerate(_graphs()):
        for kw in (dict(), dict(shared=True), dict(p=0.3)):
            got_k, lim = DC.check_op(g, DEV, H, D, seed=i + H * D, impl="kernel", worst=WORST, **kw)
            assert ops.dot_attn_last_impl == "kernel"
            got_t, _ = DC.check_op(g, DEV, H, D, seed=i + H * D, impl="tensor", worst=WORST.setdefault("tensor form", {}), **kw)
            assert ops.dot_attn_last_impl == "tensor"
            for n in got_k:                                              # the two forms against each other, under the same bounds
                assert bool(((got_k[n] - got_t[n]).abs() <= lim[n]).all()), n
    print("largest error / bound so far:", {k: (round(v, 4) if not isinstance(v, dict) else {a: round(b, 4) for a, b in v.items()}) for k, v in WORST.items()})


@pytest.mark.gpu
def test_hub_graph_and_impl_selection(monkeypatch):
    DC.check_op(_hub(), DEV, 3, 5, seed=2, impl="kernel", worst=WORST)
    g = _graphs()[5][1]
    calls = []
    real = _C.dot_attn
    monkeypatch.setattr(_C, "dot_attn", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    monkeypatch.setenv("BOT_DOT_ATTN", "tensor")                     # read at call time
    DC.check_op(g, DEV, 3, 5, seed=2)
    assert calls == [] and ops.dot_attn_last_impl == "tensor"
    monkeypatch.delenv("BOT_DOT_ATTN")
    DC.check_op(g, DEV, 3, 5, seed=2)
    assert calls == [1] and ops.dot_attn_default_impl == "kernel" and ops.dot_attn_last_impl == "kernel"
    keep33 = torch.ones(g.number_of_edges(), 33, dtype=torch.bool, device=DEV)       # one bit per head: above 32 the op runs the tensor form
    ops.dot_attention(g, torch.randn(63, 33, 2, device=DEV), *(torch.randn(200, 33, 2, device=DEV),) * 2, keep=keep33, p=0.5)
    assert ops.dot_attn_last_impl == "tensor"
    print("largest error / bound so far:", WORST)


@pytest.mark.gpu
def test_a_head_wider_than_a_tile_runs_the_tensor_form():
    H, D = WIDE
    name, g = _graphs()[5]
    q, k, v, _ = DC.normal_inputs(g.number_of_src_nodes(), g.number_of_dst_nodes(), H, D, 0)
    with pytest.raises(_C.BotKernelError, match=r"rc=-2.*does not fit"):
        _C.dot_attn(g.csc, q.to(DEV), k.to(DEV), v.to(DEV), D ** -0.5)
    DC.check_op(g, DEV, H, D, seed=1)
    assert ops.dot_attn_last_impl == "tensor"
    with pytest.raises(_C.BotKernelError):                              # the backward sweeps refuse it too
        _C.dot_attn_bwd_dst(g.csc, q.to(DEV), k.to(DEV), v.to(DEV), 1.0, None, 0.0, q.to(DEV), q.to(DEV), torch.zeros(63, 1, device=DEV))


@pytest.mark.gpu
def test_autograd_computes_each_gradient_only_when_asked(monkeypatch):
    calls = []
    real_dst, real_src = _C.dot_attn_bwd_dst, _C.dot_attn_bwd_src
    monkeypatch.setattr(_C, "dot_attn_bwd_dst", lambda *a, **k: (calls.append(("dst", k["want_dq"])), real_dst(*a, **k))[1])
    monkeypatch.setattr(_C, "dot_attn_bwd_src", lambda *a, **k: (calls.append(("src", k.get("want_dk"), k.get("want_dv"), k.get("shared", False))),
                                                                 real_src(*a, **k))[1])
    g2 = SG.small_graph(20, 30, 8).to(DEV)
    x = [torch.randn(20, 2, 4, device=DEV), torch.randn(30, 2, 4, device=DEV), torch.randn(30, 2, 4, device=DEV)]
    full = [t.clone().requires_grad_() for t in x]
    ops.dot_attention(g2, *full).sum().backward()
    calls.clear()
    g2._csr = None
    for need, seen in (((True, False, False), [("dst", True)]),):
        leaves = [t.clone().requires_grad_(r) for t, r in zip(x, need)]
        ops.dot_attention(g2, *leaves).sum().backward()
        assert calls == seen and g2._csr is None                      # the CSR is built only when k or v needs a gradient
        assert _same(leaves[0].grad, full[0].grad)
    for need, seen in (((False, True, False), ("src", True, False, False)), ((False, False, True), ("src", False, True, False))):
        calls.clear()
        leaves = [t.clone().requires_grad_(r) for t, r in zip(x, need)]
        ops.dot_attention(g2, *leaves).sum().backward()
        assert calls == [("dst", False), seen] and g2._csr is not None
        i = need.index(True)
        assert _same(leaves[i].grad, full[i].grad)
    calls.clear()
    kv = x[1].clone().requires_grad_()
    ops.dot_attention(g2, x[0], kv, kv).sum().backward()
    assert calls == [("dst", False), ("src", None, None, True)]


@pytest.mark.gpu
def test_nan_and_inf_stay_inside_the_rows_that_gather_them():
    name, g = _graphs()[6]
    src, dst = GC.positions(g)
    n_src, n_dst = g.number_of_src_nodes(), g.number_of_dst_nodes()
    q, k, v, dout = (t.to(DEV) for t in DC.normal_inputs(n_src, n_dst, 3, 5, 4))
    clean, lse = _C.dot_attn(g.csc, q, k, v, 0.5)
    u0, u1 = int(src[0]), int(src[-1])
    k2, v2 = k.clone(), v.clone()
    k2[u0, 0, 1], v2[u1, 2, 3] = float("nan"), float("inf")
    got, lse2 = _C.dot_attn(g.csc, q, k2, v2, 0.5)
    hit = torch.zeros(n_dst, dtype=torch.bool)
    hit[dst[(src == u0) | (src == u1)]] = True
    assert not bool(torch.isfinite(got[hit.to(DEV)]).all())
    assert _same(got[~hit.to(DEV)], clean[~hit.to(DEV)]) and _same(lse2[~hit.to(DEV)], lse[~hit.to(DEV)])
    iso = (GC.degree_of(dst, n_dst) == 0).to(DEV)                        # an isolated destination gives zeros
    assert int(iso.sum()) > 0 and bool((got[iso] == 0).all()) and bool((lse2[iso] == 0).all())


# ------------------------------------------------------------------------------------------------ 3. the layers
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


@pytest.mark.gpu
def test_dotgatconv_against_fp64_restatement():
    DC.check_layer(bnn.DotGatConv(8, 5, 3), DC.dotgat_conv64, _parent(), DEV, 8)
    assert ops.dot_attn_last_impl == "kernel"
    DC.check_layer(bnn.DotGatConv(8, 5, 3, allow_zero_in_degree=True), DC.dotgat_conv64, _subgraph(), DEV, 8, seed=2)
    b = _block()
    DC.check_layer(bnn.DotGatConv(8, 8, 2, allow_zero_in_degree=True), DC.dotgat_conv64, b, DEV, 8, seed=3, pair=True)
    DC.check_layer(bnn.DotGatConv(8, 4, 2, allow_zero_in_degree=True), DC.dotgat_conv64, b, DEV, 8, seed=4)
    out, a = bnn.DotGatConv(8, 4, 2).to(DEV)(_parent(), _parent().ndata["feat"], get_attention=True)
    assert a.shape == (_parent().number_of_edges(), 2, 1) and ops.dot_attn_last_impl == "tensor"


@pytest.mark.gpu
@pytest.mark.parametrize("concat", [False, True])
@pytest.mark.parametrize("beta", [False, True])
@pytest.mark.parametrize("root_weight", [False, True])
def test_transformerconv_against_fp64_restatement(concat, beta, root_weight):
    kw = dict(concat=concat, beta=beta, root_weight=root_weight)
    torch.manual_seed(0)
    DC.check_layer(DC.seeded(bnn.TransformerConv(8, 5, 3, **kw), 0), DC.transformer_conv64, _parent(), DEV, 8)
    assert ops.dot_attn_last_impl == "kernel"
    DC.check_layer(DC.seeded(bnn.TransformerConv(8, 5, 3, allow_zero_in_degree=True, **kw), 1), DC.transformer_conv64, _subgraph(), DEV, 8, seed=2)
    b = _block()
    DC.check_layer(DC.seeded(bnn.TransformerConv(8, 8, 2, bias=False, allow_zero_in_degree=True, **kw), 2), DC.transformer_conv64, b, DEV, 8, seed=3,
                   pair=True)
    DC.check_layer(DC.seeded(bnn.TransformerConv(8, 4, 1, allow_zero_in_degree=True, **kw), 3), DC.transformer_conv64, b, DEV, 8, seed=4)


@pytest.mark.gpu
def test_transformerconv_attention_dropout_against_the_same_mask(monkeypatch):
    g = _parent()
    conv = DC.seeded(bnn.TransformerConv(8, 5, 3, dropout=0.4), 0).train()
    keep = DC.draw_keep(g.number_of_edges(), 3, 0.4, 5)
    with monkeypatch.context() as m:
        m.setattr(torch, "rand", lambda *a, **k: keep.float().to(k.get("device", "cpu")))                      # rand >= p  <=>  keep
        DC.check_layer(conv, DC.transformer_conv64, g, DEV, 8, keep=keep)
    assert ops.dot_attn_last_impl == "kernel"
    x = g.ndata["feat"]
    assert not torch.equal(conv(g, x), conv(g, x)) and torch.equal(conv.eval()(g, x), conv(g, x))


# ------------------------------------------------------------------------------------------------ 4. the stack and the recipes
@pytest.mark.gpu
def test_unimp_stack_against_fp64_restatement():
    g = _parent()
    torch.manual_seed(3)
    model = bnn.UniMP(8, 5, 6, 3, 2, F.relu, norm="batch", dropout=0.5, attn_drop=0.1)
    DC.check_stack(model, g, g.ndata["feat"].cpu(), DEV)
    DC.check_stack(bnn.UniMP(8, 5, 6, 2, 2, F.relu), _subgraph(), _subgraph().ndata["feat"].cpu(), DEV)
    nids = torch.randperm(g.number_of_nodes(), generator=torch.Generator().manual_seed(3))[:600]
    _, _, blocks = next(iter(NodeDataLoader(g, nids, MultiLayerNeighborSampler([5, 7, 9]), batch_size=600, seed=4)))
    model2 = bnn.UniMP(8, 5, 6, 3, 2, F.relu, beta=False)
    DC.check_stack(model2, blocks, blocks[0].srcdata["feat"].cpu(), DEV)
    with pytest.raises(ValueError, match="edge_weight"):
        model(g, g.ndata["feat"], edge_weight=torch.ones(g.number_of_edges(), device=DEV))


def _changed(model, before):
    return all(not torch.equal(p.detach(), b) for p, b in zip(model.parameters(), before))


@pytest.mark.gpu
def test_build_unimp_full_batch_step():
    wl = workloads.build_unimp("cora", DEV)
    before = [p.detach().clone() for p in wl.model.parameters()]
    torch.manual_seed(0)
    loss, pred = wl.step()
    assert np.isfinite(float(loss.detach())) and bool(torch.isfinite(pred).all()) and _changed(wl.model, before)
    assert ops.dot_attn_last_impl == "kernel"


@pytest.mark.gpu
def test_build_unimp_sampled_epoch():
    wl = workloads.build_unimp("cora", DEV, sampled=True)
    assert wl.use_labels and "train_labels_onehot" in wl.graph.ndata
    before = [p.detach().clone() for p in wl.model.parameters()]
    torch.manual_seed(0)
    loss = wl.epoch()
    assert np.isfinite(float(torch.as_tensor(loss).detach())) and _changed(wl.model, before)
