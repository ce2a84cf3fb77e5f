"""Label reuse (n_label_iters > 0, run.py:274-279) on the fused train step, on the MI355X: bot_build_input_reuse_f32 against its numpy
restatement (tests/test_label_reuse_host.py) and against bot_build_input_f32, the whole step against the tensor-op form of the same step,
the captured step, and the one-rank partitioned step."""
import copy

import numpy as np
import pytest
import torch

from tests.test_label_reuse_host import reuse_reference

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _kernel_case(C):
    from bot_amd import _C  # noqa: F401
    gen = torch.Generator(device=DEV).manual_seed(5 + C)
    n, Fin = 5003, 7
    feat = torch.randn(n, Fin, device=DEV, generator=gen)
    pred = 3 * torch.randn(n, C, device=DEV, generator=gen)
    code = torch.where(torch.rand(n, device=DEV, generator=gen) < 0.3, torch.randint(0, C, (n,), device=DEV, generator=gen),
                       torch.full((n,), -1, device=DEV)).to(torch.int32)
    reuse = (torch.rand(n, device=DEV, generator=gen) < 0.8).to(torch.uint8)
    code[10] = code[11] = -1            # the two extreme rows take the softmax branch
    reuse[10] = reuse[11] = 1
    pred[10] = -100.0
    pred[10, 0] = 100.0                 # [100, -100, ...]
    pred[11] = 1.5                      # all equal
    return n, Fin, feat, pred, code, reuse


@pytest.mark.parametrize("C", [1, 5, 40, 128])
def test_build_input_reuse_kernel(C):
    from bot_amd import _C
    n, Fin, feat, pred, code, reuse = _kernel_case(C)
    hot = code >= 0
    soft = ~hot & (reuse != 0)
    zero = ~hot & (reuse == 0)
    assert int(hot.sum()) > 100 and int(soft.sum()) > 100 and int(zero.sum()) > 100
    # --- no row eligible for the softmax branch: build_input's output, bit for bit, without and with dropout
    none = torch.zeros_like(reuse)
    all_hot = torch.randint(0, C, (n,), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)).to(torch.int32)
    for p, seed in ((0.0, 0), (0.25, 3)):
        assert torch.equal(_C.build_input_reuse(feat, code, none, pred, C, p, seed), _C.build_input(feat, code, C, p, seed)), (C, p)
        assert torch.equal(_C.build_input_reuse(feat, all_hot, reuse, pred, C, p, seed), _C.build_input(feat, all_hot, C, p, seed)), (C, p)
        assert torch.equal(_C.build_input_reuse(feat, all_hot, None, pred, C, p, seed), _C.build_input(feat, all_hot, C, p, seed)), (C, p)
    # --- p = 0: the three kinds of label block
    calls = _C.REUSE_CALLS
    out = _C.build_input_reuse(feat, code, reuse, pred, C, 0.0, 0)
    assert _C.REUSE_CALLS == calls + 1
    assert out.shape == (n, Fin + C) and torch.equal(out[:, :Fin], feat)
    eye = torch.eye(C, device=DEV)
    assert torch.equal(out[hot][:, Fin:], eye[code[hot].long()])
    assert not out[zero][:, Fin:].any()
    ref = torch.softmax(pred.double(), -1)
    got = out[:, Fin:].double()
    err = ((got - ref).abs().amax(1) / ref.amax(1))[soft]
    print(f"build_input_reuse C={C}: softmax rows {int(soft.sum())}, worst error / row maximum {float(err.max()):.2e}")
    assert float(err.max()) <= 1e-5
    assert torch.isfinite(out[10:12]).all()
    assert float(out[10, Fin]) == 1.0 and not out[10, Fin + 1:].any()
    assert torch.allclose(out[11, Fin:], torch.full((C,), 1.0 / C, device=DEV), rtol=1e-6, atol=0)
    # the numpy restatement (exact outside the softmax rows)
    ref_np, _ = reuse_reference(feat.cpu().numpy(), code.cpu().numpy(), reuse.cpu().numpy(), pred.cpu().numpy(), C)
    o = out.cpu().numpy()
    sm = soft.cpu().numpy()
    assert np.array_equal(o[~sm], ref_np[~sm])
    np.testing.assert_allclose(o[sm], ref_np[sm], rtol=0, atol=1e-5)
    # reuse = NULL: every node without an input label takes the softmax
    out_all = _C.build_input_reuse(feat, code, None, pred, C, 0.0, 0)
    assert torch.equal(out_all[~zero], out[~zero])
    assert float(((out_all[:, Fin:].double() - ref).abs().amax(1) / ref.amax(1))[zero].max()) <= 1e-5
    # `out=`: the same bits into a given buffer (a row-strided view too), nothing outside it
    buf = torch.full((n, Fin + C + 3), 7.0, device=DEV)
    assert _C.build_input_reuse(feat, code, reuse, pred, C, 0.0, 0, out=buf[:, :Fin + C]) is not None
    assert torch.equal(buf[:, :Fin + C], out) and bool((buf[:, Fin + C:] == 7.0).all())
    # --- p = 0.25: reproducible, a stream per seed, rate, scaling, and the element masks of the restatement
    a, b, c = (_C.build_input_reuse(feat, code, reuse, pred, C, 0.25, s) for s in (3, 3, 4))
    assert torch.equal(a, b) and not torch.equal(a, c)
    _, keep = reuse_reference(feat.cpu().numpy(), code.cpu().numpy(), reuse.cpu().numpy(), pred.cpu().numpy(), C, 0.25, 3)
    keep = torch.from_numpy(keep).to(DEV)
    assert not a[~keep].any()
    share = float(keep[:, Fin:].float().mean())
    print(f"build_input_reuse C={C}: kept share of the label block {share:.4f}")
    assert abs(share - 0.75) < 0.01
    assert torch.allclose(a[keep], (out / 0.75)[keep], rtol=1e-6, atol=0)
    nz = out != 0
    assert torch.equal((a != 0), keep & nz)


def test_build_input_reuse_refusals():
    from bot_amd import _C
    n, Fin, feat, pred, code, reuse = _kernel_case(5)
    calls = _C.REUSE_CALLS
    with pytest.raises(_C.BotKernelError):
        _C.build_input_reuse(feat, code, reuse, torch.zeros(n, 129, device=DEV), 129, 0.0, 0)
    rc = _C._lib.bot_build_input_reuse_f32(feat.data_ptr(), Fin, n, Fin, 5, code.data_ptr(), reuse.data_ptr(), None, 5, 0.0, 0, None,
                                           torch.empty(n, Fin + 5, device=DEV).data_ptr(), Fin + 5, None)
    assert rc == -1
    with pytest.raises(_C.BotKernelError):
        _C.build_input_reuse(feat, code, reuse, pred[:, :3], 5, 0.0, 0)
    with pytest.raises(_C.BotKernelError):
        _C.build_input_reuse(feat, code.long(), reuse, pred, 5, 0.0, 0)
    with pytest.raises(_C.BotKernelError):
        _C.build_input_reuse(feat, code, reuse.bool(), pred, 5, 0.0, 0)
    with pytest.raises(_C.BotKernelError):
        _C.build_input_reuse(feat.cpu(), code, reuse, pred, 5, 0.0, 0)
    assert _C.REUSE_CALLS == calls          # nothing launched


# ------------------------------------------------------------------------------------------------ the whole step
def _step_setup():
    from bot_amd import synth
    ds = synth.make_dataset("arxiv", device=DEV, seed=0, scale=0.05)
    ds.graph.create_formats_()
    mask = torch.rand(ds.train_idx.shape, device=DEV, generator=torch.Generator(device=DEV).manual_seed(5)) < 0.5
    return ds, mask


def _make(kind, ds, **drops):
    import torch.nn.functional as F
    from bot_amd import nn as bnn
    C = ds.n_classes
    torch.manual_seed(0)
    if kind == "gat":
        return bnn.GAT(dim_node=ds.feat.shape[1] + C, dim_edge=0, dim_output=C, activation=F.relu, n_layers=3, n_heads=3, n_hidden=32, norm="batch",
                       linear=True, **drops).to(DEV)
    return bnn.GCN(in_feats=ds.feat.shape[1] + C, n_classes=C, n_hidden=32, n_layers=3, activation=F.relu, norm="batch", **drops).to(DEV)


def _one_step(kind, ds, mask, iters, fused_step, test_idx=None, reuse_switch=True):
    from bot_amd import _C, optim as boptim, train as T
    model = _make(kind, ds)
    opt = boptim.RMSprop(model.parameters(), lr=0.002)
    calls = _C.REUSE_CALLS
    T.FUSED_STEP, T.FUSED_REUSE = fused_step, reuse_switch
    T.DEBUG_KEEP_PREDS, T.DEBUG_PREDS[:] = True, []
    try:
        model.train()
        opt.zero_grad()
        loss, pred, _ = T.forward_backward(model, ds.graph, ds.feat, ds.labels, ds.train_idx, ds.val_idx, ds.test_idx if test_idx is None else test_idx,
                                           use_labels=True, n_label_iters=iters, loss="loge", n_classes=ds.n_classes, mask=mask)
        kept = list(T.DEBUG_PREDS)
    finally:
        T.FUSED_STEP = T.FUSED_REUSE = True
        T.DEBUG_KEEP_PREDS, T.DEBUG_PREDS[:] = False, []
    return dict(loss=loss.detach(), pred=pred.detach(), grads=[p.grad.clone() for p in model.parameters()],
                buffers={k: v.clone() for k, v in model.named_buffers()}, calls=_C.REUSE_CALLS - calls, kept=kept)


def _compare(a, b, tag):
    """a: the fused form, b: the tensor-op form; bounds of tests/test_gpu_parity.py::test_step_glue_kernels and parity_cases.fwd_close."""
    from tests.parity_cases import fwd_close
    la, lb = float(a["loss"]), float(b["loss"])
    worst = max(float((ga - gb).abs().max()) / max(float(gb.abs().max()), 1e-30) for ga, gb in zip(a["grads"], b["grads"]))
    print(f"{tag}: loss {la:.8f} / {lb:.8f} (rel {abs(la - lb) / max(1.0, abs(lb)):.2e}), max|pred diff| {float((a['pred'] - b['pred']).abs().max()):.2e}, "
          f"worst gradient error / largest entry {worst:.2e}")
    assert abs(la - lb) <= 2e-6 * max(1.0, abs(lb)), tag
    fwd_close(a["pred"], b["pred"].cpu().numpy())
    for ga, gb in zip(a["grads"], b["grads"]):
        assert float((ga - gb).abs().max()) <= 1e-5 * float(gb.abs().max()) + 1e-12, tag
    for k, v in a["buffers"].items():
        if k.endswith("num_batches_tracked"):
            assert torch.equal(v, b["buffers"][k]), (tag, k)
        else:
            w = b["buffers"][k]
            print(f"{tag}: {k} max|diff| {float((v - w).abs().max()):.2e} (largest entry {float(w.abs().max()):.2e})")
            assert torch.allclose(v, w, rtol=1e-5), (tag, k)


@pytest.mark.parametrize("kind", ["gat", "gcn"])
@pytest.mark.parametrize("iters", [1, 2])
def test_fused_label_reuse_step_matches_tensor_op_form(kind, iters):
    """S-arxiv at scale 0.05, drop rates 0, fixed mask: the fused step with n_label_iters = k against T.FUSED_STEP = False; the new wrapper
    ran k times and the reuse passes carry no autograd graph."""
    ds, mask = _step_setup()
    a = _one_step(kind, ds, mask, iters, True)
    b = _one_step(kind, ds, mask, iters, False)
    assert a["calls"] == iters and b["calls"] == 0
    assert len(a["kept"]) == iters and not any(t.requires_grad or t.grad_fn is not None for t in a["kept"])
    for k, v in a["buffers"].items():
        if k.endswith("num_batches_tracked"):
            assert int(v) == 1 + iters, k
    _compare(a, b, f"{kind} n_label_iters={iters}")


@pytest.mark.parametrize("kind", ["gat", "gcn"])
def test_nodes_outside_every_set_keep_zero_label_columns(kind):
    """A split that leaves some nodes out of train, validation and test: their membership byte is 0, their label columns stay zero in both
    forms (the reference never writes them), and the two forms agree."""
    from bot_amd import _C, train as T
    ds, mask = _step_setup()
    te = ds.test_idx[:-200].clone()
    out_nodes = ds.test_idx[-200:]
    m = T._reuse_members(ds.feat.shape[0], ds.train_idx, ds.val_idx, te)
    assert m is not None and not m[out_nodes].any() and int(m.sum()) == ds.feat.shape[0] - 200
    code = torch.full((ds.feat.shape[0],), -1, dtype=torch.int32, device=DEV)
    x = _C.build_input_reuse(ds.feat, code, m, torch.randn(ds.feat.shape[0], ds.n_classes, device=DEV), ds.n_classes, 0.0, 0)
    assert not x[out_nodes][:, ds.feat.shape[1]:].any() and bool((x[ds.val_idx][:, ds.feat.shape[1]:].sum(1) > 0.99).all())
    a = _one_step(kind, ds, mask, 1, True, test_idx=te)
    b = _one_step(kind, ds, mask, 1, False, test_idx=te)
    assert a["calls"] == 1
    _compare(a, b, f"{kind} with 200 nodes in no set")
    full = _one_step(kind, ds, mask, 1, True)
    assert not torch.equal(full["pred"], a["pred"])                 # the left-out nodes' columns matter


def test_label_reuse_with_the_reference_drop_rates():
    """dropout 0.75 / input dropout 0.25 / attention dropout 0.1 and the step's own random split: three steps, three finite, different losses;
    every pass draws its own input-dropout seed."""
    from bot_amd import _C, optim as boptim, train as T
    ds, _ = _step_setup()
    torch.manual_seed(1)
    model = _make("gat", ds, input_drop=0.25, dropout=0.75, attn_drop=0.1)
    opt = boptim.RMSprop(model.parameters(), lr=0.002)
    calls = _C.REUSE_CALLS
    ls = [float(T.train_step(model, ds.graph, ds.feat, ds.labels, ds.train_idx, ds.val_idx, ds.test_idx, opt, use_labels=True, n_label_iters=2,
                             loss="loge", n_classes=ds.n_classes)[0]) for _ in range(3)]
    print("losses with the reference's drop rates, n_label_iters = 2:", ls)
    assert _C.REUSE_CALLS - calls == 6
    assert all(np.isfinite(v) for v in ls) and len(set(ls)) == 3


@pytest.mark.parametrize("kind", ["gat", "gcn"])
def test_default_step_did_not_move(kind):
    """n_label_iters = 0: loss, pred and gradients are bit for bit those of a run with the new path switched off (FUSED_REUSE = False)."""
    ds, mask = _step_setup()
    a = _one_step(kind, ds, mask, 0, True, reuse_switch=True)
    b = _one_step(kind, ds, mask, 0, True, reuse_switch=False)
    assert a["calls"] == 0 and b["calls"] == 0
    assert torch.equal(a["loss"], b["loss"]) and torch.equal(a["pred"], b["pred"])
    for ga, gb in zip(a["grads"], b["grads"]):
        assert torch.equal(ga, gb)


# ------------------------------------------------------------------------------------------------ captured, traced, partitioned
def _capture_case(drops, iters=1):
    from bot_amd import train as T
    ds, mask = _step_setup()
    m1 = _make("gat", ds, **drops)
    m2 = _make("gat", ds, **drops)
    m2.load_state_dict(copy.deepcopy(m1.state_dict()))
    o1 = torch.optim.RMSprop(m1.parameters(), lr=0.002, capturable=True)
    o2 = torch.optim.RMSprop(m2.parameters(), lr=0.002, capturable=True)
    kw = dict(use_labels=True, n_label_iters=iters, loss="loge", n_classes=ds.n_classes)
    if not drops:
        kw["mask"] = mask

    def eager():
        return T.train_step(m1, ds.graph, ds.feat, ds.labels, ds.train_idx, ds.val_idx, ds.test_idx, o1, **kw)
    cap = T.captured_train_step(m2, ds.graph, ds.feat, ds.labels, ds.train_idx, ds.val_idx, ds.test_idx, o2, warmup=3, **kw)
    import weakref
    cap.watched = (weakref.ref(m2), weakref.ref(o2))    # this function's own references to the captured model and optimizer end here
    return eager, cap


@pytest.mark.isolated
def test_captured_label_reuse_step_replays():
    """captured_train_step(n_label_iters=1): drop rates 0 and a fixed mask - three replays, each loss equal to the eager step's on a copy of
    the model within 2e-6 relative; with the reference's drop rates three replays give three different losses (every pass's baked seed is
    moved by the SEED_OFFSET word)."""
    from bot_amd import _C
    calls = _C.REUSE_CALLS
    eager, cap = _capture_case({})
    assert _C.REUSE_CALLS - calls == 4          # three warm-up steps and the capture pass
    import gc
    gc.collect()
    # the graph replays onto the addresses of its model's parameters and its optimizer's state: the captured step keeps both alive
    assert all(r() is not None for r in cap.watched)
    for _ in range(3):                          # the capture ran 3 warm-up steps on its model
        eager()
    for it in range(3):
        le, _ = eager()
        lc, _ = cap()
        torch.cuda.synchronize()
        print(f"replay {it}: captured loss {float(lc):.8f}, eager {float(le):.8f}")
        assert abs(float(lc) - float(le)) <= 2e-6 * max(1.0, abs(float(le))), it
    _C.SEED_OFFSET = None
    _, cap = _capture_case(dict(input_drop=0.25, dropout=0.75, attn_drop=0.1))
    ls = []
    for _ in range(3):
        lc, _ = cap()
        torch.cuda.synchronize()
        ls.append(float(lc))
    print("captured losses with the reference's drop rates:", ls)
    assert all(np.isfinite(v) for v in ls) and len(set(ls)) == 3
    _C.SEED_OFFSET = None


@pytest.mark.isolated
def test_no_multi_workgroup_torch_reduction_in_label_reuse_step(tmp_path):
    """The rule of test_no_multi_workgroup_torch_reduction_in_capturable_steps for the new step: the kernel trace of one eager step with
    n_label_iters = 1 shows no `at::native::reduce_kernel` launch with grid[1] > 1 (the softmax lives in bot_build_input_reuse_f32, not in
    a torch reduction) - and the new kernel is in it."""
    import json
    from torch.profiler import ProfilerActivity, profile
    from bot_amd import optim as boptim, train as T
    ds, mask = _step_setup()
    model = _make("gat", ds)
    opt = boptim.RMSprop(model.parameters(), lr=0.002)

    def eager():
        return T.train_step(model, ds.graph, ds.feat, ds.labels, ds.train_idx, ds.val_idx, ds.test_idx, opt, use_labels=True, n_label_iters=1,
                            loss="loge", n_classes=ds.n_classes, mask=mask)
    eager()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        eager()
        torch.cuda.synchronize()
    path = str(tmp_path / "trace.json")
    prof.export_chrome_trace(path)
    evs = [e for e in json.load(open(path))["traceEvents"] if e.get("cat") == "kernel"]
    assert len(evs) > 10, "no kernel records in the trace"
    assert sum("build_input_reuse_kernel" in e["name"] for e in evs) == 1
    assert not any("softmax" in e["name"].lower() for e in evs), [e["name"][:80] for e in evs if "softmax" in e["name"].lower()]
    red = [e for e in evs if "at::native::reduce_kernel" in e["name"]]
    with_grid = [e for e in red if "grid" in e.get("args", {})]
    multi = [(e["name"][:120], e["args"]["grid"]) for e in with_grid if int(e["args"]["grid"][1]) > 1]
    print(f"label reuse step: {len(evs)} kernels, {len(red)} torch reduce_kernel launches ({len(with_grid)} with grid info), multi-workgroup: {multi}")
    assert len(with_grid) == len(red), "the trace carries no grid sizes: cannot tell single- from multi-workgroup reductions"
    assert not multi, multi


@pytest.mark.isolated
def test_one_rank_partitioned_label_reuse_step():
    """bot_amd.dist.forward_backward(n_label_iters=1) on one rank (RCCL group, SyncBatchNorm) takes the new path and agrees with the
    single-GPU tensor-op form."""
    import torch.distributed as dist
    from bot_amd import _C, dist as bdist, optim as boptim, train as T
    from tests.test_gpu_parity import init_one_rank_rccl
    init_one_rank_rccl()
    try:
        ds, _ = _step_setup()
        n = ds.feat.shape[0]
        coin = torch.rand(n, device=DEV, generator=torch.Generator(device=DEV).manual_seed(9)) < 0.5      # per node: the partition sorts its indices
        b = _one_step("gat", ds, coin[ds.train_idx], 1, False)
        part = bdist.partition_dataset(ds, 0, 1, DEV, None)
        assert part.node_ids is None and torch.equal(part.train_idx, torch.sort(ds.train_idx).values)
        mask = coin[part.train_idx]
        model = bdist.wrap_model(_make("gat", ds), None)
        opt = boptim.RMSprop(model.parameters(), lr=0.002)
        model.train()
        opt.zero_grad()
        calls = _C.REUSE_CALLS
        loss, pred = bdist.forward_backward(model, part, use_labels=True, n_label_iters=1, loss="loge", n_classes=ds.n_classes, mask=mask)
        assert _C.REUSE_CALLS - calls == 1
        a = dict(loss=loss.detach(), pred=pred.detach(), grads=[p.grad.clone() for p in model.parameters()], buffers={})
        _compare(a, b, "one-rank partitioned, n_label_iters=1")
        for k, v in model.named_buffers():
            if k.endswith("num_batches_tracked"):
                assert int(v) == 2, k
    finally:
        dist.destroy_process_group()
