"""R-GCN on the MI355X: the two relation sweeps of csrc/spmm_rel.hip against the float64 restatement (tests/rgcn_cases.py) - entry for
entry in the exact regime (integer-valued operands, a norm of powers of two, coefficients in quarters: sums that are exact in float32
whatever their order), whole rows and chunked rows alike, and under bounds derived from row lengths and rounding counts on seeded normal
inputs, the kernel form and the tensor form - then `nn.RelGraphConv` and `nn.RGCN` against their float64 restatements under the suite's
own criteria (tests/parity_cases.py), and the steps of `workloads.build_rgcn`.

Largest error seen as a fraction of its derived bound (run with -s to print them): DESIGN §8 "R-GCN"."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from bot_amd import _C, minibatch, ops, workloads
from bot_amd import nn as bnn
from bot_amd.errors import DGLError
from bot_amd.sampling import ClusterLoader, MultiLayerNeighborSampler, NodeDataLoader, cluster_assignment, sample_block
from tests import block_cases as BC
from tests import rgcn_cases as RC
from tests import sage_cases as SG

pytestmark = pytest.mark.gpu
DEV = "cuda"
# Per width two relation shapes (R, B; B None: one-hot), thinned so that every width and every shape appears, each on every graph of
# _graphs() (whole rows, long rows, blocks).  Widths: 1 the smallest; 3, 5 odd, 4-byte lanes; 4, 40, 64 one group of 8 / 16 lanes; 65 an
# odd width beyond a wavefront of 4-byte lanes (tiles); 256 the workload's; 1000 walks tiles of 16-byte lanes.  Shapes: (40, 17) and
# one-hot 17 run two passes of 16 blocks; (5, 3) pads a pass of 4.
CASES = {1: ((1, 1), (40, 17)), 3: ((5, 2), (17, None)), 4: ((5, 3), (40, 16)), 5: ((40, 16), (5, None)), 40: ((40, 17), (5, 2)),
         64: ((5, None), (40, 16)), 65: ((17, None), (5, 3)), 256: ((1, 1), (5, 2)), 1000: ((5, 3), (5, None))}
WIDTHS = tuple(CASES)
WORST = {}


@functools.lru_cache(maxsize=None)
def _graphs():
    """(name, graph on the device): 1 / 63 / 64 / 65 square rows with isolated rows and parallel edges, chunk = 4 variants (long rows in
    both directions: the workspace and the combine at small sizes), and a block with n_src > n_dst (tests/test_gated_gpu.py's)."""
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


def _same_bytes(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _wide(t, pad, fill=7.0):
    """A device view of `t` ([n, ...], rows flattened) whose rows sit in a buffer `pad` floats wider, and the buffer."""
    n, w = t.shape[0], int(np.prod(t.shape[1:]))
    buf = torch.full((n, w + pad), fill, dtype=torch.float32, device=DEV)
    buf[:, :w].copy_(t.reshape(n, w).to(DEV))
    return buf[:, :w].view(t.shape), buf


def _check_strided(g, case, R, pad):
    """The two entry points on operands and outputs that are column blocks of wider buffers: the bytes of the contiguous call, and the
    sentinel in the padding survives."""
    coef = None if case["coef"] is None else case["coef"].to(DEV)
    Bc = R if coef is None else coef.shape[1]
    n_dst, Fw = g.number_of_dst_nodes(), case["x"].shape[1]
    csc = g.csc
    et = RC.position_order(g, case["et"]).to(DEV, torch.int32).contiguous()
    nm = RC.position_order(g, case["norm"]).to(DEV).contiguous()
    x, y = case["x"].to(DEV), case["y"].to(DEV)
    Z = _C.spmm_rel_expand(csc, x, et, R, coef, nm)
    o = _C.spmm_rel_contract(csc, y, et, R, coef, nm)
    zv, zbuf = _wide(torch.full((n_dst, Bc, Fw), 9.0), pad, 9.0)
    ov, obuf = _wide(torch.full((n_dst, Fw), 9.0), pad, 9.0)
    _C.spmm_rel_expand(csc, _wide(x, pad)[0], et, R, coef, nm, out=zv)
    _C.spmm_rel_contract(csc, _wide(y, pad)[0], et, R, coef, nm, out=ov)
    assert _same_bytes(zv, Z) and _same_bytes(ov, o), (Fw, R, Bc, pad)
    assert bool((zbuf[:, Bc * Fw:] == 9.0).all()) and bool((obuf[:, Fw:] == 9.0).all())
    return Z, o


# ------------------------------------------------------------------------------------------------ 1. exact
@pytest.mark.parametrize("Fw", WIDTHS)
def test_exact_regime_fp64_entry_for_entry(Fw):
    """Forward and all gradients equal the float64 restatement bit for bit on every graph; norm=None gives the bytes of a norm of ones;
    two calls give the same bytes; strided operands give the bytes of contiguous ones."""
    for i, (name, g) in enumerate(_graphs()):
        for j, (R, B) in enumerate(CASES[Fw]):
            case = RC.exact_case(g, Fw, R, B, seed=17 * i + Fw + j)
            got = RC.check_exact(g, case, DEV, "kernel")
            again = RC.run_ops(g, case, DEV, "kernel")
            assert all(torch.equal(got[k], again[k]) for k in got), (name, R, B)
            none = RC.run_ops(g, case, DEV, "kernel", norm=False)
            ones = RC.run_ops(g, dict(case, norm=torch.ones(g.number_of_edges())), DEV, "kernel")
            assert all(torch.equal(none[k], ones[k]) for k in none), (name, R, B)
            for pad in (3, 4):
                Z, o = _check_strided(g, case, R, pad)
                assert torch.equal(Z.cpu().double(), got["Z"]) and torch.equal(o.cpu().double(), got["out"])


def test_two_pass_shapes_run_the_sixteen_block_instances():
    g = _graphs()[5][1]
    for (R, B), expand, contract in (((40, 17), "spmm_rel_expand_kernel<0,16,", "spmm_rel_contract_kernel<0,16,"),
                                     ((17, None), "spmm_rel_expand_kernel<1,16,", "spmm_rel_contract_kernel<1,1,"),
                                     ((5, 3), "spmm_rel_expand_kernel<0,4,", "spmm_rel_contract_kernel<0,4,")):
        case = RC.exact_case(g, 4, R, B, seed=5)
        et = RC.position_order(g, case["et"]).to(DEV, torch.int32).contiguous()
        coef = None if B is None else case["coef"].to(DEV)
        _C.spmm_rel_expand(g.csc, case["x"].to(DEV), et, R, coef)
        assert expand in _C._lib.bot_last_kernel().decode()
        _C.spmm_rel_contract(g.csc, case["y"].to(DEV), et, R, coef)
        assert contract in _C._lib.bot_last_kernel().decode()


def test_exact_regime_fp64_on_the_hub_graph():
    """Rows above 2 048 in-edges at the default chunk; the ranges are shrunk so that every sum's absolute terms stay below the limit."""
    g = _hub()
    RC.check_exact(g, RC.exact_case(g, 4, 3, 1, seed=3, lim=1), DEV, "kernel")
    RC.check_exact(g, RC.exact_case(g, 4, 3, None, seed=4, lim=1), DEV, "kernel")


# ------------------------------------------------------------------------------------------------ 2. rounded, and the two forms
@pytest.mark.parametrize("Fw", WIDTHS)
def test_kernel_and_tensor_forms_against_fp64_under_derived_bounds(Fw):
    """Both sweeps over the CSC, their gradients (the other sweep over the CSR) and dcoef on seeded normal inputs."""
    for i in (3, 4, 5, 6):
        name, g = _graphs()[i]
        for j, (R, B) in enumerate(CASES[Fw]):
            case = RC.normal_case(g, Fw, R, B, seed=i + Fw + j)
            got_k = RC.check_bounds(g, case, DEV, "kernel", WORST)
            got_t = RC.check_bounds(g, case, DEV, "tensor", WORST)
            lim = RC.bounds(g, case)
            for k in got_k:                                            # the two forms agree within the sum of their bounds
                assert bool(((got_k[k] - got_t[k]).abs() <= 2 * lim[k]).all()), (name, k)
            RC.check_bounds(g, case, DEV, "kernel", WORST, norm=False)
    print("largest error / bound so far:", {k: round(v, 4) for k, v in sorted(WORST.items())})
    assert all(v <= 1.0 for v in WORST.values())


def test_hub_graph_against_fp64_under_derived_bounds():
    g = _hub()
    RC.check_bounds(g, RC.normal_case(g, 4, 3, 1, seed=2), DEV, "kernel", WORST)
    RC.check_bounds(g, RC.normal_case(g, 4, 3, None, seed=3), DEV, "kernel", WORST)
    print("largest error / bound so far:", {k: round(v, 4) for k, v in sorted(WORST.items())})
    assert all(v <= 1.0 for v in WORST.values())


def test_impl_selection_is_read_at_call_time(monkeypatch):
    g = _graphs()[5][1]
    case = RC.normal_case(g, 5, 5, 2, seed=2)
    calls = []
    real = _C.spmm_rel_expand
    monkeypatch.setattr(_C, "spmm_rel_expand", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    run = lambda **kw: ops.rel_expand_sum(g, case["x"].to(DEV), case["et"].to(DEV), 5, case["coef"].to(DEV), **kw)
    monkeypatch.setenv("BOT_REL", "tensor")
    out_t = run()
    assert calls == []
    out_k = run(impl="kernel")                                        # the argument wins over the variable
    assert calls == [1] and float((out_k - out_t).abs().max()) < 1e-4
    monkeypatch.delenv("BOT_REL")
    run()
    assert len(calls) == (2 if ops.rel_default_impl == "kernel" else 1)


def test_needed_gradients_only_and_nothing_kept_under_no_grad(monkeypatch):
    calls = []
    real_e, real_c, real_d, real_s = _C.spmm_rel_expand, _C.spmm_rel_contract, _C.sddmm_dot_blocks, _C.sddmm_dot
    monkeypatch.setattr(_C, "spmm_rel_expand", lambda *a, **k: (calls.append("expand"), real_e(*a, **k))[1])
    monkeypatch.setattr(_C, "spmm_rel_contract", lambda *a, **k: (calls.append("contract"), real_c(*a, **k))[1])
    monkeypatch.setattr(_C, "sddmm_dot_blocks", lambda *a, **k: (calls.append("dots"), real_d(*a, **k))[1])
    monkeypatch.setattr(_C, "sddmm_dot", lambda *a, **k: (calls.append("dots"), real_s(*a, **k))[1])
    g0 = SG.small_graph(20, 30, 8)
    case = RC.normal_case(g0, 8, 5, 2, seed=1)
    full = {}
    for op, inp, fwd, bwd in ((ops.rel_expand_sum, "x", "expand", "contract"), (ops.rel_contract_sum, "y", "contract", "expand")):
        for need_t, need_c in ((True, True), (True, False), (False, True), (False, False)):
            g2 = SG.small_graph(20, 30, 8).to(DEV)
            calls.clear()
            t = case[inp].clone().to(DEV).requires_grad_(need_t)
            coef = case["coef"].clone().to(DEV).requires_grad_(need_c)
            out = op(g2, t, case["et"].to(DEV), 5, coef, case["norm"].to(DEV), impl="kernel")
            if need_t or need_c:
                out.sum().backward()
            else:
                assert out.grad_fn is None
            assert calls == [fwd] + ([bwd] if need_t else []) + (["dots"] if need_c else []), (inp, need_t, need_c, calls)
            assert (g2._csr is None) == (not need_t)                  # the CSR is built only for the source-side gradient
            if need_t and need_c:
                full[inp] = (t.grad, coef.grad)
            else:                                                    # a subset gives the bytes of the full backward
                assert t.grad is None or _same_bytes(t.grad, full[inp][0])
                assert coef.grad is None or _same_bytes(coef.grad, full[inp][1])
    # under no_grad the autograd context - the only place the forward keeps anything - does not outlive the call, whatever
    # save_for_backward was handed; with gradients it lives on as the result's grad_fn
    import gc
    import weakref
    g2 = SG.small_graph(20, 30, 8).to(DEV)
    for fn, op, inp in ((ops._RelExpand, ops.rel_expand_sum, "x"), (ops._RelContract, ops.rel_contract_sum, "y")):
        ctxs = []
        real = fn.forward
        monkeypatch.setattr(fn, "forward", staticmethod(lambda ctx, *a, real=real, ctxs=ctxs: (ctxs.append(weakref.ref(ctx)), real(ctx, *a))[1]))
        t = case[inp].to(DEV).requires_grad_()
        coef = case["coef"].to(DEV).requires_grad_()
        with torch.no_grad():
            out = op(g2, t, case["et"].to(DEV), 5, coef, impl="kernel")
        gc.collect()
        assert out.grad_fn is None and not out.requires_grad and len(ctxs) == 1 and ctxs[0]() is None
        kept = op(g2, t, case["et"].to(DEV), 5, coef, impl="kernel")
        gc.collect()
        assert ctxs[1]() is kept.grad_fn and kept.grad_fn is not None
    assert g2._csr is None


def test_relations_are_checked_once_per_graph_and_tensor(monkeypatch):
    g = SG.small_graph(20, 30, 8).to(DEV)
    case = RC.normal_case(g, 4, 5, 2, seed=1)
    et, x, coef = case["et"].to(DEV), case["x"].to(DEV), case["coef"].to(DEV)
    ops.rel_expand_sum(g, x, et, 5, coef)
    reads = []
    real = torch.Tensor.tolist
    monkeypatch.setattr(torch.Tensor, "tolist", lambda self: (reads.append(1), real(self))[1])
    ops.rel_expand_sum(g, x, et, 5, coef)
    ops.rel_contract_sum(g, case["y"].to(DEV), et, 5, coef)
    assert reads == []
    et[0] = 5                                                        # an in-place change is a new version: checked again
    with pytest.raises(DGLError, match="num_rels = 5"):
        ops.rel_expand_sum(g, x, et, 5, coef)


# ------------------------------------------------------------------------------------------------ 3. the layer
@functools.lru_cache(maxsize=None)
def _parent():
    g = BC.parent_graph(DEV, n=4000, e_raw=30000)
    g.edata["etype"] = RC.relations(g, 5, 9).to(DEV)
    g.edata["norm"] = bnn.rel_norm(g, "etype", 5)
    return g


@functools.lru_cache(maxsize=None)
def _block():
    g = _parent()
    seeds = torch.randperm(g.number_of_nodes(), generator=torch.Generator().manual_seed(2))[:700].to(DEV, torch.int32)
    b = sample_block(g, seeds, 5, 77)
    assert b.number_of_src_nodes() > b.number_of_dst_nodes()
    return b


@pytest.mark.parametrize("order", ["aggregate", "project"])
@pytest.mark.parametrize("num_bases", [2, None])
def test_relgraphconv_against_fp64_restatement(order, num_bases):
    kw = dict(order=order, num_bases=num_bases)
    g, b = _parent(), _block()
    RC.check_conv(g, DEV, 8, 5, 5, **kw)
    RC.check_conv(g, DEV, 8, 64, 5, seed=1, bias=False, activation=F.elu, self_loop=False, with_norm=False, **kw)
    RC.check_conv(g, DEV, 64, 8, 5, seed=2, layer_norm=True, activation=F.relu, **kw)
    RC.check_conv(g.subgraph(torch.arange(0, 4000, 3, device=DEV)), DEV, 8, 6, 5, seed=5, **kw)
    RC.check_conv(b, DEV, 8, 6, 5, seed=3, pair=True, with_norm=False, **kw)
    RC.check_conv(b, DEV, 8, 4, 5, seed=4, layer_norm=True, **kw)


def test_relgraphconv_through_the_halves_gemm():
    """At the workload's width the dense product of either order runs on the fp16-halves GEMM where it pays (bot_amd.gemm)."""
    from bot_amd import gemm
    old = gemm.MIN_ROWS
    gemm.MIN_ROWS = 1024
    try:
        for order in ("aggregate", "project"):
            RC.check_conv(_parent(), DEV, 128, 128, 5, seed=6, num_bases=2, order=order)
    finally:
        gemm.MIN_ROWS = old


# ------------------------------------------------------------------------------------------------ 4. the stack and the recipes
def test_rgcn_stack_against_fp64_restatement():
    g = _parent()
    torch.manual_seed(3)
    model = bnn.RGCN(8, 5, 6, 3, 5, F.relu, num_bases=2, norm="batch", dropout=0.5)
    RC.check_stack(model, g, g.ndata["feat"].cpu(), DEV)
    nids = torch.randperm(g.number_of_nodes(), generator=torch.Generator().manual_seed(3))[:600]
    _, _, blocks = next(iter(NodeDataLoader(g, nids, MultiLayerNeighborSampler([5, 7, 9]), batch_size=600, seed=4)))
    model2 = bnn.RGCN(8, 5, 6, 3, 5, F.relu, regularizer=None)
    RC.check_stack(model2, blocks, blocks[0].srcdata["feat"].cpu(), DEV)


def _moved(model, before):
    return all(not torch.equal(p.detach(), q) for p, q in zip(model.parameters(), before))


@pytest.mark.parametrize("name,scale,regularizer", [("cora", 1.0, "basis"), ("arxiv", 0.05, "basis"), ("cora", 1.0, None)])
def test_build_rgcn_full_batch_steps_and_cluster_epoch(name, scale, regularizer):
    wl = workloads.build_rgcn(name, DEV, scale=scale, regularizer=regularizer, drop=False)
    before = [p.detach().clone() for p in wl.model.parameters()]
    torch.manual_seed(0)
    losses = [float(torch.as_tensor(wl.step()[0]).detach()) for _ in range(2)]
    assert all(np.isfinite(v) for v in losses) and _moved(wl.model, before)
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in wl.model.parameters())
    ds, g = wl.dataset, wl.graph
    g.ndata["feat"] = ds.feat
    before = [p.detach().clone() for p in wl.model.parameters()]
    loader = ClusterLoader(g, cluster_assignment(g, 8, "random", seed=2), parts_per_batch=4, seed=0)
    loss, skipped = minibatch.train_epoch_subgraphs(wl.model, loader, wl.optimizer, ds.labels, ds.train_idx, val_idx=ds.val_idx, test_idx=ds.test_idx,
                                                    step_kw=wl.step_kw)
    assert np.isfinite(loss) and _moved(wl.model, before)


@pytest.mark.parametrize("name,scale", [("cora", 1.0), ("arxiv", 0.05)])
def test_build_rgcn_sampled_epoch(name, scale):
    wl = workloads.build_rgcn(name, DEV, sampled=True, scale=scale, drop=False)
    before = [p.detach().clone() for p in wl.model.parameters()]
    torch.manual_seed(0)
    loss = float(torch.as_tensor(wl.epoch()).detach())
    assert np.isfinite(loss) and _moved(wl.model, before)


# ------------------------------------------------------------------------------------------------ 5. errors
def test_error_paths():
    name, g = _graphs()[3]
    n, E = g.number_of_nodes(), g.number_of_edges()
    case = RC.normal_case(g, 8, 5, 2, seed=1)
    x, y, et, coef, nm = (case[k].to(DEV) for k in ("x", "y", "et", "coef", "norm"))
    assert ops.rel_expand_sum(g, x, et, 5, coef, nm).shape == (n, 2, 8) and ops.rel_contract_sum(g, y, et, 5, coef, nm).shape == (n, 8)
    for fn, bad, text in ((ops.rel_expand_sum, (x[:-1], et, 5, coef), f"({n - 1}, 8)"), (ops.rel_contract_sum, (y[:, :1], et, 5, coef), f"({n}, 1, 8)"),
                          (ops.rel_expand_sum, (x, et.cpu(), 5, coef), "cpu"), (ops.rel_expand_sum, (x, et, 5, coef.cpu()), "cpu"),
                          (ops.rel_expand_sum, (x, et, 5, coef, nm.cpu()), "cpu"), (ops.rel_expand_sum, (x.double(), et, 5, coef.double()), "float64"),
                          (ops.rel_expand_sum, (x, et, 3, None), "num_rels = 3"), (ops.rel_contract_sum, (y, et + 4, 5, coef), "num_rels = 5")):
        with pytest.raises(DGLError) as err:
            fn(g, *bad)
        assert text in str(err.value), (text, str(err.value))
    part = BC.parent_graph(DEV, n=200, e_raw=1500, seed=7)
    part.halo = object()                                              # a partition's block carries a halo plan
    with pytest.raises(ValueError, match="partition"):
        ops.rel_contract_sum(part, torch.randn(200, 1, 4, device=DEV), torch.zeros(part.number_of_edges(), dtype=torch.int64, device=DEV), 1)
    etp = RC.position_order(g, case["et"]).to(DEV, torch.int32).contiguous()
    with pytest.raises(_C.BotKernelError, match="unit inner stride"):
        _C.spmm_rel_expand(g.csc, x.t().contiguous().t(), etp, 5, coef)
    with pytest.raises(_C.BotKernelError, match="contiguous"):
        _C.spmm_rel_contract(g.csc, y.transpose(1, 2).contiguous().transpose(1, 2), etp, 5, coef)
    with pytest.raises(_C.BotKernelError, match="positions"):
        _C.spmm_rel_expand(g.csc, x, etp[:-1].contiguous(), 5, coef)
    with pytest.raises(_C.BotKernelError, match="int32"):
        _C.spmm_rel_expand(g.csc, x, etp.long(), 5, coef)
    out = bnn.RelGraphConv(8, 4, 5, self_loop=False, bias=False).to(DEV)(g, x, et)
    assert bool((out[g.in_degrees() == 0] == 0).all())                # every fifth node of the graph has no in-edges
