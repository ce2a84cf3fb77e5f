"""APPNP / GCNII on the MI355X: one `bot_appnp_step_f32` sweep (csrc/appnp.hip) against the float64 restatement of one step
(tests/appnp_cases.py), the exact pins (bit identity with the propagation step at p = 0, the regenerated mask, dropped edges), the op
forward and backward against the restatement under the carried bound, the kernel form against the tensor form, the memory claim, and
the layers and workloads."""
import numpy as np
import pytest
import torch

import bot_amd
from bot_amd import _C, minibatch, ops, smoothing, workloads
from bot_amd import nn as bnn
from tests import appnp_cases as AC
from tests import smooth_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = AC.U
INF = float("inf")

_GRAPHS = {}
WORST = {"step": 0.0, "op": 0.0, "forms": 0.0}       # the largest observed fractions of the bounds (README "APPNP and GCNII")


def _gpu_graph(name):
    if name not in _GRAPHS:
        if name == "hub":
            from tests.test_subgraph_gpu import _hub_graph
            g = _hub_graph()
            src, dst = (t.cpu() for t in g.edges())
            _GRAPHS[name] = (g, src, dst, g.number_of_nodes())
        else:
            src, dst, n = SC.graph(name)
            _GRAPHS[name] = (bot_amd.Graph(src, dst, n).to(DEV), src, dst, n)
    return _GRAPHS[name]


def _note(key, frac):
    WORST[key] = max(WORST[key], frac)
    print(f"APPNP_FRAC {key} {frac:.4f} (largest so far {WORST[key]:.4f})")


def _frac(got, want, bound):
    err = (got.cpu().double() - want).abs()
    assert bool((err[bound == 0] == 0).all())
    return float((err / bound.clamp(min=1e-300)).max()) if err.numel() else 0.0


# ------------------------------------------------------------------------------------------------ 1. one launch against the restatement
def _view(n, C, strided, values):
    """A [n, C] float32 view on the device over a buffer filled with the sentinel 777: contiguous, a column slice at an odd offset of an
    odd pitch (4-byte lanes), or one at a 16-byte aligned offset of a pitch that is a multiple of 4 floats.  values None: 555 inside."""
    if strided == 0:
        base, off = torch.empty(n, C), 0
    elif strided == 1:
        base, off = torch.empty(n, C + 5), 3
    else:
        base, off = torch.empty(n, (C + 3) // 4 * 4 + 8), 4
    base.fill_(777.0)
    base[:, off:off + C] = 555.0 if values is None else values
    base = base.to(DEV)
    return base[:, off:off + C], base, off


def _untouched(base, off, C):
    back = base.cpu()
    back[:, off:off + C] = 777.0
    return bool((back == 777.0).all())


def _check_step(name, C, seed, *, strided, y0, ss, ds, osc, acc, ew, p, transposed):
    """One launch against AC.step in float64 under (deg + 8 + [ew] + [p > 0]) 2^-24 mag per entry; out_scale: the bound times the factor
    plus 2^-24 of the product (tests/test_smooth_gpu._check_step); acc_out: the bound plus 2^-24 (|acc_in| + |o|).  acc: None, "new" (a
    buffer of its own), "inplace" (acc_in is acc_out) or "y" (acc_in is y).  transposed: the sweep runs over the CSR with pos = csr2csc.
    Nothing outside the views is written and two calls give equal bytes."""
    g, src, dst, n = _gpu_graph(name)
    csc, csr, c2c = AC.directions(src, dst)
    rows, cols, eid = csr if transposed else csc
    d = g.csr if transposed else g.csc
    assert torch.equal(d.indices.cpu().long(), cols) and (not transposed or torch.equal(g.csr2csc.cpu().long(), c2c))
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda: torch.randn(n, C, generator=gen)
    vec = lambda: 0.5 + torch.rand(n, generator=gen)
    yv = rnd()
    y, _, _ = _view(n, C, strided, yv)
    y0v = rnd() if y0 else None
    y0d = _view(n, C, (strided + 1) % 3 if strided else 0, y0v)[0] if y0 else None
    ssv, dsv, oscv = (vec() if f else None for f in (ss, ds, osc))
    ewv = (0.5 + torch.rand(rows.numel(), generator=gen)) if ew else None          # per position of the direction swept
    acc_v = None if acc is None else (yv if acc == "y" else rnd())
    a, b, step_no, sd = 0.9, 0.1, 5, 1234567 + seed
    dv = lambda t: None if t is None else t.to(DEV).contiguous()
    pos = g.csr2csc if transposed else None
    deg = torch.bincount(rows, minlength=n)

    def launch():
        out, ob, off = _view(n, C, strided, None)
        if acc is None:
            ai = ao = abase = None
        elif acc == "inplace":
            ao, abase, _ = _view(n, C, strided, acc_v)
            ai = ao
        else:
            ao, abase, _ = _view(n, C, strided, None)
            ai = y if acc == "y" else _view(n, C, 0, acc_v)[0]
        got = _C.appnp_step(d, y, out, a, b, y0=y0d, src_scale=dv(ssv), dst_scale=dv(dsv), out_scale=dv(oscv), acc_in=ai, acc_out=ao, ew=dv(ewv),
                            pos=pos, p=p, seed=sd, step=step_no)
        assert got is out and _untouched(ob, off, C) and (abase is None or _untouched(abase, off, C))
        return out, ao
    out, ao = launch()
    kernel = _C._lib.bot_last_kernel().decode()
    o, want, acc_want, mag = AC.step(rows, cols, n, yv, a=a, b=b, y0=y0v, src_scale=ssv, dst_scale=dsv, out_scale=oscv, acc_in=acc_v, ew=ewv,
                                     q=c2c if transposed else None, p=p, seed=sd, step_no=step_no)
    tol = AC.step_tol(deg, mag, ew, p)
    tol_o = tol if oscv is None else tol * oscv.double()[:, None] + U * want.abs()
    frac = _frac(out, want, tol_o)
    if acc is not None:
        frac = max(frac, _frac(ao, acc_want, tol + U * (acc_v.double().abs() + o.abs())))
    _note("step", frac)
    assert frac <= 1.0, (name, C, kernel, frac)
    out2, ao2 = launch()
    assert torch.equal(out2.view(torch.int32), out.view(torch.int32))
    assert acc is None or torch.equal(ao2.view(torch.int32), ao.view(torch.int32))
    return kernel


_COMBOS = (dict(strided=0, y0=True, ss=True, ds=True, osc=False, acc=None, ew=False, p=0.0, transposed=False),
           dict(strided=1, y0=False, ss=False, ds=True, osc=True, acc="new", ew=True, p=0.5, transposed=True),
           dict(strided=2, y0=True, ss=True, ds=False, osc=True, acc="inplace", ew=False, p=0.5, transposed=False),
           dict(strided=0, y0=False, ss=False, ds=False, osc=False, acc="y", ew=True, p=0.0, transposed=True),
           dict(strided=2, y0=True, ss=True, ds=True, osc=True, acc="new", ew=True, p=0.5, transposed=True))


@pytest.mark.parametrize("C", [1, 3, 4, 7, 40, 47, 112, 260, 1024])
def test_step_against_fp64_restatement_of_one_step(C):
    """The isolated-node graph (300 rows, parallel edges): every C takes another lane layout; the combos cover every operand present and
    absent, p in {0, 0.5}, pos NULL and a real csr2csc over the CSR."""
    g, src, dst, n = _gpu_graph("tiny")
    pairs = src * n + dst
    assert int((torch.bincount(dst, minlength=n) == 0).sum()) >= 3 and pairs.unique().numel() < pairs.numel()     # isolated rows, parallel edges
    kernels = {_check_step("tiny", C, C + i, **kw) for i, kw in enumerate(_COMBOS)}
    assert all(k.startswith("bot::appnp_step_kernel<") for k in kernels), kernels
    assert any(k.endswith("ew,drop>") for k in kernels) and any(k.endswith("-,->") for k in kernels), kernels


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_step_against_fp64_restatement_row_counts(n):
    name = f"pl{n}"
    if name not in _GRAPHS:
        src, dst = SC.powerlaw_graph(n, 4 * n, 40 + n, n_isolated=1)
        _GRAPHS[name] = (bot_amd.Graph(src, dst, n).to(DEV), src, dst, n)
    for C in (3, 40):
        for i, kw in enumerate(_COMBOS):
            _check_step(name, C, n + C + i, **kw)


@pytest.mark.parametrize("C,combo", [(8, 4), (7, 1), (8, 2), (7, 0)])
def test_step_against_fp64_restatement_on_the_hub_graph(C, combo):
    """Largest in-degree above 2048: the hub rows run as chunks of the row plan and are combined in slot order, in both directions."""
    g, src, dst, n = _gpu_graph("hub")
    assert int(torch.bincount(dst).max()) > 2048 and g.csc.n_long > 0 and g.csr.n_long > 0
    _check_step("hub", C, C + combo, **_COMBOS[combo])


# ------------------------------------------------------------------------------------------------ 2. exact pins
@pytest.mark.parametrize("name,C", [("tiny", 7), ("tiny", 40), ("tiny", 260), ("hub", 8), ("hub", 7)])
def test_p_zero_is_bit_identical_to_the_propagation_step(name, C):
    g, src, dst, n = _gpu_graph(name)
    gen = torch.Generator().manual_seed(C)
    y, y0 = torch.randn(n, C, generator=gen).to(DEV), torch.randn(n, C, generator=gen).to(DEV)
    sc = [(0.5 + torch.rand(n, generator=gen)).to(DEV) for _ in range(3)]
    for ss, ds, osc in ((sc[0], sc[1], None), (None, sc[1], sc[2]), (sc[0], None, None), (None, None, None)):
        want = _C.propagate_step(g.csc, y, y0, torch.empty_like(y), 0.9, 0.1, ss, ds, -INF, INF, out_scale=osc)
        got = _C.appnp_step(g.csc, y, torch.empty_like(y), 0.9, 0.1, y0=y0, src_scale=ss, dst_scale=ds, out_scale=osc)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_mask_on_a_ring_graph_forward_and_backward():
    """Every row one in-edge, E = N = 1000, y = 1, no scales, a = 1: the output IS m_k per position - the numpy mask, forward over the CSC
    and backward over the CSR through pos."""
    n, p, seed, step_no = 1000, 0.5, 987654321987, 3
    src = torch.arange(n)
    g = bot_amd.Graph(src, (src + 1) % n, n).to(DEV)
    keep = torch.from_numpy(AC.keep_mask(seed, step_no, n, p))
    m = torch.where(keep, torch.tensor(1.0 / (1.0 - p)), torch.tensor(0.0))
    y = torch.ones(n, 4, device=DEV)
    fwd = _C.appnp_step(g.csc, y, torch.empty_like(y), 1.0, p=p, seed=seed, step=step_no).cpu()
    assert torch.equal(fwd, m[:, None].expand(n, 4))                               # row v holds position v
    bwd = _C.appnp_step(g.csr, y, torch.empty_like(y), 1.0, pos=g.csr2csc, p=p, seed=seed, step=step_no).cpu()
    assert torch.equal(bwd, m[g.csr2csc.cpu().long()][:, None].expand(n, 4))      # row u holds the edge u -> u + 1: CSC position csr2csc[u]
    assert 0 < int(keep.sum()) < n
    assert torch.equal(ops.appnp_keep(seed, step_no, n, p, DEV).cpu(), keep)       # the torch mask on the device


def test_a_dropped_edge_with_a_nan_source_leaves_its_destination_finite():
    g, src, dst, n = _gpu_graph("tiny")
    (rows, cols, _), _, _ = AC.directions(src, dst)
    p, seed, step_no = 0.5, 42, 1
    keep = torch.from_numpy(AC.keep_mask(seed, step_no, rows.numel(), p))
    u = int(cols[torch.nonzero(~keep)[0, 0]])                                      # the source of a dropped position
    from_u = cols == u
    poisoned = torch.zeros(n, dtype=torch.bool)
    poisoned[rows[from_u & keep]] = True
    spared = torch.zeros(n, dtype=torch.bool)
    spared[rows[from_u & ~keep]] = True
    spared &= ~poisoned
    assert bool(spared.any())
    for bad in (float("nan"), INF):
        for C in (7, 260):                                                          # narrow lane groups (predicated loads) and 64-lane groups (scalar branch)
            y = torch.randn(n, C, generator=torch.Generator().manual_seed(C))
            y[u] = bad
            y0 = torch.zeros(n, C, device=DEV)
            out = _C.appnp_step(g.csc, y.to(DEV), torch.empty(n, C, device=DEV), 0.9, 0.1, y0=y0, p=p, seed=seed, step=step_no).cpu()
            finite = torch.isfinite(out).all(1)
            assert torch.equal(finite, ~poisoned) and bool(finite[spared].all())


# ------------------------------------------------------------------------------------------------ 3. the op
def _scales(g, src, dst, n, ew):
    """The package's float32 scales (what the kernel multiplies by), checked against the exact ones: pow and the division are correctly
    rounded to within 2 ulp, a float32 sum of deg weights to within deg ulp."""
    ws = smoothing._weights(g, None if ew is None else ew.to(DEV))
    ss, ds = (t.cpu() for t in smoothing._degree_scales(g, "DAD", ws))
    w = torch.ones(src.numel(), dtype=torch.float64) if ew is None else ew.double()
    deg = torch.zeros(n, dtype=torch.float64).index_add_(0, dst, w)
    deg = torch.where(deg > 0, deg, torch.ones((), dtype=torch.float64))
    slack = (2 + (torch.bincount(dst, minlength=n).double() if ew is not None else 0)) * U
    assert bool(((ss.double() - deg ** -0.5).abs() <= slack * deg ** -0.5).all())
    return ss, ds


@pytest.mark.parametrize("k", [1, 2, 10])
@pytest.mark.parametrize("C", [7, 40])
@pytest.mark.parametrize("name", ["tiny", "small"])
def test_op_against_fp64_restatement_under_the_carried_bound(name, C, k):
    """Forward and (dx, dh0) of the kernel form within the carried bound of the float64 restatement, the tensor form with the same seed
    within twice that bound of the kernel form, two calls equal bytes; alpha in {0.1, 0.5}, edge_drop in {0, 0.5}, h0 shared and
    separate, with and without an edge weight."""
    g, src, dst, n = _gpu_graph(name)
    gen = torch.Generator().manual_seed(100 * k + C)
    x, h0v, dout = (torch.randn(n, C, generator=gen) for _ in range(3))
    ewv = 0.5 + torch.rand(src.numel(), generator=gen)
    for ew in (None, ewv):
        ss, ds = _scales(g, src, dst, n, ew)
        ewd = None if ew is None else ew.to(DEV)
        for alpha in (0.1, 0.5):
            for p in (0.0, 0.5):
                for shared in (True, False):
                    seed = 31 * k + int(100 * alpha) + int(shared)
                    r = AC.propagate(src, dst, n, x, None if shared else h0v, k, alpha, ss, ds, p=p, seed=seed, ew=ew, dout=dout)

                    def run(impl):
                        xd = x.to(DEV).requires_grad_()
                        hd = None if shared else h0v.to(DEV).requires_grad_()
                        y = ops.appnp_propagate(g, xd, k, alpha, h0=hd, edge_drop=p, seed=seed, edge_weight=ewd, impl=impl)
                        y.backward(dout.to(DEV))
                        return y.detach(), xd.grad, None if shared else hd.grad
                    ker, ten, again = run("kernel"), run("tensor"), run("kernel")
                    pairs = [(0, "h", "Eh"), (1, "dx", "Edx")] + ([] if shared else [(2, "dh0", "Edh0")])
                    frac = max(_frac(ker[i], r[v], r[e]) for i, v, e in pairs)
                    _note("op", frac)
                    assert frac <= 1.0, (name, C, k, alpha, p, shared, ew is not None, frac)
                    fr2 = max(_frac(ten[i], ker[i].cpu().double(), 2 * r[e]) for i, v, e in pairs)
                    _note("forms", fr2)
                    assert fr2 <= 1.0, (name, C, k, alpha, p, shared, ew is not None, fr2)
                    assert all(torch.equal(again[i].view(torch.int32), ker[i].view(torch.int32)) for i, _, _ in pairs)


def test_kernel_form_saves_nothing_of_size_n_times_c():
    """Under saved_tensors_hooks the kernel form saves no tensor with numel >= N C; the tensor form saves at least k of them."""
    g, src, dst, n = _gpu_graph("small")
    C, k = 8, 10
    x = torch.randn(n, C, device=DEV)

    def saved_big(impl, h0):
        sizes = []
        xd = x.clone().requires_grad_()
        with torch.autograd.graph.saved_tensors_hooks(lambda t: sizes.append(t.numel()) or t, lambda t: t):
            y = ops.appnp_propagate(g, xd, k, 0.1, h0=h0, edge_drop=0.5, seed=5, impl=impl)
        y.sum().backward()
        return sum(s >= n * C for s in sizes)
    for h0 in (None, torch.randn(n, C, device=DEV, requires_grad=True)):
        assert saved_big("kernel", h0) == 0
        assert saved_big("tensor", h0) >= k


def test_subgraph_is_accepted_and_odd_widths_are_padded():
    g, src, dst, n = _gpu_graph("small")
    sub = g.subgraph(torch.arange(0, n, 2, device=DEV))
    ssrc, sdst = (t.cpu() for t in sub.edges())
    m = sub.number_of_nodes()
    x = torch.randn(m, 41, generator=torch.Generator().manual_seed(1))
    ss, ds = _scales(sub, ssrc, sdst, m, None)
    r = AC.propagate(ssrc, sdst, m, x, None, 3, 0.1, ss, ds, p=0.5, seed=9, dout=torch.ones(m, 41))
    xd = x.to(DEV).requires_grad_()
    y = ops.appnp_propagate(sub, xd, 3, 0.1, edge_drop=0.5, seed=9, impl="kernel")
    y.sum().backward()
    assert y.shape == (m, 41) and xd.grad.shape == (m, 41)
    assert _frac(y.detach(), r["h"], r["Eh"]) <= 1.0 and _frac(xd.grad, r["dx"], r["Edx"]) <= 1.0


# ------------------------------------------------------------------------------------------------ 4. layers and workloads
def _close(got, want, what):
    """The project's parameter-gradient criterion: within 1.0e-5 of the reference's largest entry."""
    assert float((got.cpu().double() - want).abs().max()) <= 1e-5 * float(want.abs().max()), what


@pytest.mark.parametrize("project", [True, False])
def test_gcn2conv_against_the_restatement(project):
    from tests.test_appnp_host import _gcn2_case, gcn2_grads
    _, coo, conv, feat, feat_0, dout = _gcn2_case(project, 7, activation=torch.tanh)
    g = _gpu_graph("tiny")[0]
    (out, got), (ref, want) = gcn2_grads(conv.to(DEV), g, coo, feat.to(DEV), feat_0.to(DEV), dout.to(DEV), project, activation=torch.tanh)
    _close(out, ref, "out")
    for k in want:
        _close(got[k], want[k], k)


@pytest.mark.parametrize("train", [False, True])
def test_appnpconv_against_the_restatement(train):
    g, src, dst, n = _gpu_graph("tiny")
    conv = bnn.APPNPConv(10, 0.1, edge_drop=0.5).to(DEV).train(train)
    gen = torch.Generator().manual_seed(11)
    x, dout = torch.randn(n, 40, generator=gen), torch.randn(n, 40, generator=gen)
    torch.manual_seed(21)
    seed = ops.new_dropout_seed(0.5)                       # what the layer draws from torch's generator
    torch.manual_seed(21)
    xd = x.to(DEV).requires_grad_()
    out = conv(g, xd)
    out.backward(dout.to(DEV))
    ss, ds = _scales(g, src, dst, n, None)
    r = AC.propagate(src, dst, n, x, None, 10, 0.1, ss, ds, p=0.5 if train else 0.0, seed=seed, dout=dout)
    _close(out.detach(), r["h"], "out")
    _close(xd.grad, r["dx"], "dx")


@pytest.mark.parametrize("build", [workloads.build_appnp, workloads.build_gcn2])
def test_workload_step_and_subgraph_step(build):
    wl = build("cora", DEV)
    loss = wl.step()[0]
    assert np.isfinite(float(loss.detach()))
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in wl.model.parameters())
    ds, g = wl.dataset, wl.graph
    n = g.number_of_nodes()
    roles = minibatch.node_roles(n, ds.train_idx, ds.val_idx, ds.test_idx)
    g.ndata["feat"] = ds.feat
    sub = g.subgraph(torch.arange(0, n, 2, device=DEV))
    res = minibatch.subgraph_step(wl.model, sub, wl.optimizer, ds.labels, roles, step_kw=wl.step_kw)
    assert res is not None and np.isfinite(float(res[0].detach()))
