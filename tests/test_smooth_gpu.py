"""Correct and Smooth on the MI355X: one `bot_propagate_step_f32` sweep (csrc/propagate.hip) against the float64 restatement of one
step (tests/smooth_cases.py), full `LabelPropagation` / `CorrectAndSmooth` runs against the float64 restatement, the kernel form against
the tensor form, subgraphs, blocks, and `evaluate_smoothed` on S-cora."""
import math

import pytest
import torch

import bot_amd
from bot_amd import _C, sampling, smoothing, train, workloads
from tests import smooth_cases as SC

pytestmark = pytest.mark.gpu
DEV = "cuda"
# Full runs: every entry within 1.0e-5 ABSOLUTE of the float64 restatement - the project's logit criterion; the values lie in [-1, 2].
TOL = 1.0e-5
U = 2.0 ** -24           # unit roundoff of float32

_GRAPHS = {}


def _gpu_graph(name):
    if name not in _GRAPHS:
        src, dst, n = SC.graph(name)
        _GRAPHS[name] = bot_amd.Graph(src, dst, n).to(DEV)
    return _GRAPHS[name]


# ------------------------------------------------------------------------------------------------ 1. one step against the restatement
def _view(n, C, strided, fill, gen):
    """A [n, C] float32 view on the device and its backing buffer: contiguous, a column slice at an odd offset of an odd pitch (4-byte
    lanes), or a column slice at a 16-byte aligned offset of a pitch that is a multiple of 4 floats (keeps the lane width C allows)."""
    if strided == 0:
        base = torch.empty(n, C)
        off = 0
    elif strided == 1:
        base, off = torch.empty(n, C + 5), 3
    else:
        base, off = torch.empty(n, (C + 3) // 4 * 4 + 8), 4
    base.fill_(777.0)
    base[:, off:off + C] = torch.randn(n, C, generator=gen) if fill else 555.0
    base = base.to(DEV)
    return base[:, off:off + C], base, off


def _check_step(g, src, dst, C, *, strided, fixed, row_abs, clamp, adj, seed, out_scale=False):
    """One launch against SC.step in float64.  Bound per entry: the row's sum is a chain of deg fused multiply-adds, then one product
    for alpha * dst_scale, one for beta * y0 and one more fma, so |error| <= gamma_(deg + 4) * (alpha dst_scale sum |src_scale y| +
    |beta y0|) with gamma_k ~ k 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1; a long row's chunks
    only shorten the chains); (deg + 8) 2^-24 is used.  The clamp is 1-Lipschitz and fixed rows are copies.  row_abs adds a sum of C
    terms: the entries' bounds plus (C + 8) 2^-24 of the exact norm.  out_scale multiplies the stored row once more: the bound times
    the factor plus 2^-24 of the product; fixed rows and row_abs are those of the unscaled result."""
    n = g.number_of_nodes()
    d = g.csc
    gen = torch.Generator().manual_seed(seed)
    y, _, _ = _view(n, C, strided, True, gen)
    y0, _, _ = _view(n, C, (strided + 1) % 3 if strided else 0, True, gen)
    out, out_base, off = _view(n, C, strided, False, gen)
    deg = torch.bincount(dst, minlength=n)
    degf = deg.float().clamp(min=1)
    ss, ds = {"DAD": (degf ** -0.5, degf ** -0.5), "DA": (None, 1.0 / degf), "AD": (1.0 / degf, None), None: (None, None)}[adj]
    fx = (torch.rand(n, generator=gen) < 0.3) if fixed else None
    lo, hi = (-0.25, 0.5) if clamp else (-math.inf, math.inf)
    alpha, beta = 0.8, 0.2
    ref, ref_abs, mag = SC.step(src, dst, y.cpu(), y0.cpu(), alpha, beta, ss, ds, lo, hi, fx)
    dv = lambda t: None if t is None else t.to(DEV).contiguous()
    ra = torch.full((n,), -1.0, device=DEV) if row_abs else None
    osc = (0.5 + torch.rand(n, generator=gen)) if out_scale else None
    kw = dict(fixed=None if fx is None else dv(fx.to(torch.uint8)), out_scale=dv(osc))
    got = _C.propagate_step(d, y, y0, out, alpha, beta, dv(ss), dv(ds), lo, hi, row_abs=ra, **kw)
    assert got is out
    o = out.cpu().double()
    tol = (deg.double()[:, None] + 8) * U * mag
    want = ref if osc is None else ref * osc.double()[:, None]
    tol_o = tol if osc is None else tol * osc.double()[:, None] + U * want.abs()
    bad = (o - want).abs() > tol_o
    assert not bool(bad.any()), (C, adj, torch.nonzero(bad)[:5].tolist(), (o - want).abs().max().item())
    if fx is not None:
        assert torch.equal(out.cpu()[fx], y0.cpu()[fx] if osc is None else y0.cpu()[fx] * osc[fx][:, None])
    if clamp and fx is None and osc is None:
        assert o.min() >= lo and o.max() <= hi
    back = out_base.cpu()                                   # nothing outside the [n, C] view was written
    back[:, off:off + C] = 777.0
    assert bool((back == 777.0).all())
    if row_abs:
        tol_abs = tol.sum(1) + (C + 8) * U * ref_abs
        assert bool(((ra.cpu().double() - ref_abs).abs() <= tol_abs).all()), (C, adj, (ra.cpu().double() - ref_abs).abs().max().item())
    # two calls give identical bytes
    out2 = torch.empty_like(out_base)[:, off:off + C]
    ra2 = torch.empty(n, device=DEV) if row_abs else None
    _C.propagate_step(d, y, y0, out2, alpha, beta, dv(ss), dv(ds), lo, hi, row_abs=ra2, **kw)
    assert torch.equal(out2.view(torch.int32), out.view(torch.int32))
    if row_abs:
        assert torch.equal(ra2.view(torch.int32), ra.view(torch.int32))
    return _C._lib.bot_last_kernel().decode()


_COMBOS = (dict(strided=0, fixed=True, row_abs=True, clamp=True, adj="DAD"),
           dict(strided=1, fixed=False, row_abs=False, clamp=False, adj="AD", out_scale=True),
           dict(strided=2, fixed=True, row_abs=True, clamp=False, adj="DA", out_scale=True),
           dict(strided=0, fixed=False, row_abs=True, clamp=True, adj=None))


@pytest.mark.parametrize("C", [1, 3, 4, 7, 40, 41, 47, 112, 260, 514, 1023, 1024])
def test_step_kernel_against_fp64_restatement_of_one_step(C):
    """The isolated-node graph (300 rows: several workgroups at every lane-group width); every C takes another lane layout: 4- / 8- /
    16-byte lanes, groups of 8 / 16 / 32 / 64 lanes, 1 to 16 register chunks per lane."""
    src, dst, n = SC.graph("tiny")
    g = _gpu_graph("tiny")
    assert int((torch.bincount(dst, minlength=n) == 0).sum()) >= 3
    kernels = {_check_step(g, src, dst, C, seed=C + i, **kw) for i, kw in enumerate(_COMBOS)}
    assert all(k.startswith("bot::prop_step_kernel<") for k in kernels), kernels
    if C % 4 == 0:
        assert len(kernels) == 2, kernels               # the odd-pitch slice takes 4-byte lanes, the others 16-byte lanes


@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_step_kernel_against_fp64_restatement_row_counts(n):
    src, dst = SC.powerlaw_graph(n, 4 * n, 40 + n, n_isolated=1)
    g = bot_amd.Graph(src, dst, n).to(DEV)
    for C in (3, 40, 47):
        for i, kw in enumerate(_COMBOS):
            _check_step(g, src, dst, C, seed=n + C + i, **kw)


@pytest.mark.parametrize("C,combo", [(8, 0), (7, 1), (13, 2)])
def test_step_kernel_against_fp64_restatement_on_the_hub_graph(C, combo):
    """Largest in-degree above 2048: the hub rows run as chunks of the row plan and are combined in slot order."""
    from tests.test_subgraph_gpu import _hub_graph
    if "hub" not in _GRAPHS:
        _GRAPHS["hub"] = _hub_graph()
    g = _GRAPHS["hub"]
    src, dst = (t.cpu() for t in g.edges())
    assert int(torch.bincount(dst).max()) > 2048 and g.csc.n_long > 0
    _check_step(g, src, dst, C, seed=C, **_COMBOS[combo])


# ------------------------------------------------------------------------------------------------ 2. full runs against the restatement
def _cpu_tensor_error(name, C, adj, autoscale, ref):
    """The fp32 tensor form on the CPU against the same float64 result: the error a plain fp32 implementation has on this fixture."""
    src, dst, n = SC.graph(name)
    y_soft, y_true, mask = SC.cs_inputs(name, C)
    cs = smoothing.CorrectAndSmooth(correction_adj=adj, smoothing_adj=adj, autoscale=autoscale)
    return (cs(bot_amd.Graph(src, dst, n), y_soft, y_true, mask).double() - ref).abs().max().item()


@pytest.mark.parametrize("autoscale", [True, False])
@pytest.mark.parametrize("adj", ["DAD", "DA", "AD"])
@pytest.mark.parametrize("C", [7, 40])
@pytest.mark.parametrize("name", ["small", "large"])
def test_correct_and_smooth_against_fp64_restatement(name, C, adj, autoscale):
    """50 + 50 iterations at alpha 0.8 on the 3 000-node / 12 000-edge and the 20 000-node / 137 000-edge power-law fixtures.
    Criterion: every entry within 1.0e-5 absolute of the float64 restatement (the project's logit criterion; the values lie in
    [-1, 2]).  The fp32 tensor form on the CPU is measured on the same fixture and printed beside the kernel's error; on these
    fixtures it was at most 6.5e-7, the kernel form at most 4.1e-7.  Before comparing: no row's raw autoscale factor lies within 1 %
    of the 1000 threshold."""
    ref, raw = SC.cs_reference(name, C, adj, autoscale)
    assert SC.scale_margin(raw) > 0.01, "a raw autoscale factor lies within 1 % of the threshold: choose another seed"
    g = _gpu_graph(name)
    y_soft, y_true, mask = (t.to(DEV) for t in SC.cs_inputs(name, C))
    cs = smoothing.CorrectAndSmooth(correction_adj=adj, smoothing_adj=adj, autoscale=autoscale, impl="kernel")
    got = cs(g, y_soft, y_true, mask)
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == y_soft.shape
    err = (got.cpu().double() - ref).abs().max().item()
    cpu_err = _cpu_tensor_error(name, C, adj, autoscale, ref)
    print(f"C&S {name} C={C} {adj} autoscale={autoscale}: kernel max |diff| = {err:.3e}, fp32 tensor form on the CPU {cpu_err:.3e}, "
          f"autoscale margin {SC.scale_margin(raw):.3f}")
    assert err <= TOL
    assert torch.equal(cs(g, y_soft, y_true, mask), got)            # the same bytes from call to call


@pytest.mark.parametrize("adj", ["DAD", "DA", "AD"])
@pytest.mark.parametrize("C", [7, 40])
@pytest.mark.parametrize("name", ["small", "large"])
def test_label_propagation_against_fp64_restatement(name, C, adj):
    """`LabelPropagation(50, 0.8, adj)` from int64 labels under a mask, same criterion (1.0e-5 absolute)."""
    labels, ref = SC.lp_reference(name, C, adj)
    _, _, mask = SC.cs_inputs(name, C)
    g = _gpu_graph(name)
    got = smoothing.LabelPropagation(50, 0.8, adj, impl="kernel")(g, labels.to(DEV), mask=mask.to(DEV))
    err = (got.cpu().double() - ref).abs().max().item()
    src, dst, n = SC.graph(name)
    cpu_err = (smoothing.LabelPropagation(50, 0.8, adj)(bot_amd.Graph(src, dst, n), labels, mask=mask).double() - ref).abs().max().item()
    print(f"LP {name} C={C} {adj}: kernel max |diff| = {err:.3e}, fp32 tensor form on the CPU {cpu_err:.3e}")
    assert got.shape == (n, C) and err <= TOL


# ------------------------------------------------------------------------------------------------ 3. kernel form against tensor form
@pytest.mark.parametrize("autoscale", [True, False])
@pytest.mark.parametrize("adj", ["DAD", "DA", "AD"])
@pytest.mark.parametrize("name,C", [("small", 7), ("small", 47), ("large", 40)])
def test_kernel_form_against_tensor_form_on_the_gpu(name, C, adj, autoscale):
    """Both forms on the device, 1.0e-5 absolute between them; C = 47 runs padded to 48 columns in both."""
    assert SC.scale_margin(SC.cs_reference(name, C, adj, autoscale)[1]) > 0.01
    g = _gpu_graph(name)
    y_soft, y_true, mask = (t.to(DEV) for t in SC.cs_inputs(name, C))
    kw = dict(correction_adj=adj, smoothing_adj=adj, autoscale=autoscale)
    a = smoothing.CorrectAndSmooth(impl="kernel", **kw)(g, y_soft, y_true, mask)
    b = smoothing.CorrectAndSmooth(impl="tensor", **kw)(g, y_soft, y_true, mask)
    err = (a - b).abs().max().item()
    print(f"kernel vs tensor {name} C={C} {adj} autoscale={autoscale}: max |diff| = {err:.3e}")
    assert a.shape == b.shape == y_soft.shape and err <= TOL
    assert smoothing.default_impl(y_soft) in ("kernel", "tensor")
    post = (mask[:50], "fix")
    lk = smoothing.LabelPropagation(20, 0.5, adj, impl="kernel")(g, 2 * y_soft - 0.5, mask=mask, post_step=post)
    lt = smoothing.LabelPropagation(20, 0.5, adj, impl="tensor")(g, 2 * y_soft - 0.5, mask=mask, post_step=post)
    assert (lk - lt).abs().max().item() <= TOL and torch.equal(lk[mask[:50]], (2 * y_soft - 0.5)[mask[:50]])


def test_correct_and_smooth_makes_no_host_read():
    g = _gpu_graph("small")
    y_soft, y_true, mask = (t.to(DEV) for t in SC.cs_inputs("small", 7))
    member = SC.member(g.number_of_nodes(), mask.cpu()).to(DEV)
    order = torch.argsort(mask)
    for impl in ("kernel", "tensor"):
        for autoscale in (True, False):
            cs = smoothing.CorrectAndSmooth(5, 0.8, "DAD", 5, 0.8, "DA", autoscale=autoscale, impl=impl)
            want = cs(g, y_soft, y_true, mask)              # (builds the graph's structures and the cached degree vectors)
            torch.cuda.synchronize()
            torch.cuda.set_sync_debug_mode("error")
            try:
                got = cs.smooth(g, cs.correct(g, y_soft, y_true, mask), y_true, mask)
                got_bool = cs(g, y_soft, y_true[order], member)
            finally:
                torch.cuda.set_sync_debug_mode("default")
            assert torch.equal(got, want) and torch.equal(got_bool, want)


# ------------------------------------------------------------------------------------------------ 4. graphs
def test_subgraph_is_accepted_and_block_is_refused():
    g = _gpu_graph("small")
    n = g.number_of_nodes()
    nodes = torch.randperm(n, generator=torch.Generator().manual_seed(3))[:1200]
    sub = sampling.node_subgraph(g, nodes.to(DEV))
    src, dst = (t.cpu() for t in sub.edges())
    y_soft, y_true, mask = SC.cs_inputs("small", 7)
    ys = y_soft[nodes]
    known = torch.arange(0, 1200, 4)
    labels = torch.randint(0, 7, (known.numel(),), generator=torch.Generator().manual_seed(4))
    ref, raw = SC.correct_and_smooth(src, dst, 1200, ys, labels, known, autoscale=False)
    got = smoothing.CorrectAndSmooth(autoscale=False, impl="kernel")(sub, ys.to(DEV), labels.to(DEV), known.to(DEV))
    assert (got.cpu().double() - ref).abs().max().item() <= TOL
    block = sampling.sample_block(g, torch.arange(64, device=DEV, dtype=torch.int32), 5, seed=1)
    assert block.is_block
    with pytest.raises(ValueError, match="square"):
        smoothing.CorrectAndSmooth(impl="kernel")(block, y_soft.to(DEV), y_true.to(DEV), mask.to(DEV))
    with pytest.raises(ValueError, match="square"):
        smoothing.LabelPropagation(3, 0.5)(block, y_soft.to(DEV))
    y = y_soft.to(DEV)
    with pytest.raises(_C.BotKernelError, match="alias"):    # out == y is refused before any launch
        _C.propagate_step(g.csc, y, y.clone(), y, 0.5, 0.5, None, None, 0.0, 1.0)


# ------------------------------------------------------------------------------------------------ 5. evaluate_smoothed
def test_evaluate_smoothed_on_s_cora():
    """S-cora at a quarter of its size, the untrained GCN.  Smoothing with D^-1 A at alpha 0.4: P is row-stochastic and every entry
    stays in [0, 1], so a training row keeps at least 0.6 at its label and at most 0.4 anywhere else - its argmax is the label."""
    wl = workloads.build("cora", DEV, scale=0.25, drop=False)
    ds = wl.dataset
    cs = smoothing.CorrectAndSmooth(10, 0.8, "DAD", 10, 0.4, "DA")
    out = smoothing.evaluate_smoothed(wl.model, wl.graph, ds.feat, ds.labels, ds.train_idx, ds.val_idx, ds.test_idx, cs,
                                      use_labels=False, loss="logit", n_classes=ds.n_classes)
    assert len(out) == 7
    accs, smoothed = out[:6], out[6]
    assert all(isinstance(a, float) and math.isfinite(a) and 0.0 <= a <= 1.0 for a in accs), accs
    assert smoothed.shape == (wl.n_nodes, ds.n_classes) and smoothed.is_cuda and bool(torch.isfinite(smoothed).all())
    assert torch.equal(smoothed[ds.train_idx].argmax(1), ds.labels[ds.train_idx, 0])
    assert accs[3] == 1.0
    base = train.evaluate(wl.model, wl.graph, ds.feat, ds.labels, ds.train_idx, ds.val_idx, ds.test_idx, use_labels=False, loss="logit",
                          n_classes=ds.n_classes)
    assert all(abs(a - float(b)) < 1e-6 for a, b in zip(accs[:3], base[:3]))
