"""Label reuse on the fused train step (run.py:274-279), without a GPU: bot_build_input_reuse_f32 is exported, bound and validates its
arguments; its contract restated in numpy (tests/test_label_reuse_gpu.py holds the kernel to it, dropout masks element by element); and the
Python control flow of the new path - `forward_backward(n_label_iters=k)` over a torch stand-in for the one new wrapper - against the
tensor-op form of the same step."""
import ctypes

import numpy as np
import pytest
import torch

from tests.test_sampling_host import philox4x32_10

M64 = (1 << 64) - 1


# ------------------------------------------------------------------------------------------------ the kernel's contract, in numpy
def reuse_reference(feat, code, reuse, pred, C, p=0.0, seed=0, seed_offset=None):
    """include/bot_gnn.h bot_build_input_reuse_f32 -> (out float32 [N, F + C], keep bool [N, F + C]).  Softmax in float64 (the kernel's is
    fp32: callers compare with a tolerance); everything else is exact: the one-hot rows, the zero rows, the feature columns, the mask."""
    feat = np.asarray(feat, dtype=np.float32)
    n, F = feat.shape
    W = F + C
    code = np.asarray(code)
    x = np.zeros((n, W), dtype=np.float64)
    x[:, :F] = feat
    hot = code >= 0
    x[np.nonzero(hot)[0], F + code[hot]] = 1.0
    soft = ~hot if reuse is None else (~hot & (np.asarray(reuse) != 0))
    z = np.asarray(pred, dtype=np.float64)[:, :C]
    e = np.exp(z - z.max(axis=1, keepdims=True))
    x[soft, F:] = (e / e.sum(axis=1, keepdims=True))[soft]
    keep = np.ones((n, W), dtype=bool)
    if p > 0:
        s = int(seed) & M64
        if seed_offset is not None:
            s = (s + int(seed_offset) * 0x9E3779B97F4A7C15) & M64
        nquad = (W + 3) // 4
        words = philox4x32_10(s, np.arange(n * nquad, dtype=np.uint64)).reshape(n, nquad * 4)[:, :W]
        u = (words >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)
        keep = ~(u < np.float32(p))
        x = np.where(keep, x * float(np.float32(1.0) / (np.float32(1.0) - np.float32(p))), 0.0)
    return x.astype(np.float32), keep


# ------------------------------------------------------------------------------------------------ the CPU stand-in for the one new wrapper
CALLS = [0]


def build_input_reuse_standin(feat, code, reuse, pred, n_classes, p, seed, out=None):
    """_C.build_input_reuse with torch CPU ops (tests/_oracle_backend.py has the stand-ins of the other wrappers: dropout from torch's
    generator there too, exact with p = 0)."""
    n, F = feat.shape
    block = torch.zeros(n, n_classes)
    hot = code >= 0
    rows = torch.nonzero(hot)[:, 0]
    block[rows, code[rows].long()] = 1.0
    soft = ~hot if reuse is None else (~hot & (reuse != 0))
    block = torch.where(soft[:, None], torch.softmax(pred[:, :n_classes].detach().float(), dim=-1), block)
    x = torch.cat([feat, block], 1)
    if p > 0:
        keep = torch.rand(x.shape, generator=torch.Generator().manual_seed(int(seed) % (2 ** 31))) >= p
        x = torch.where(keep, x / (1.0 - p), torch.zeros_like(x))
    CALLS[0] += 1
    if out is not None:
        out.copy_(x)
        return out
    return x


def install_standin():
    """For spawned worker processes (after _oracle_backend.install_direct()): the stand-in and the test-only switch."""
    from bot_amd import _C, train as T
    _C.build_input_reuse = build_input_reuse_standin
    T.FORCE_REUSE = True


@pytest.fixture()
def reuse_backend(monkeypatch):
    from bot_amd import _C, train as T
    from bot_amd.nn import fused
    from tests import _oracle_backend
    _oracle_backend.install(monkeypatch)
    monkeypatch.setattr(_C, "build_input_reuse", build_input_reuse_standin)
    monkeypatch.setattr(T, "FORCE_REUSE", True)
    monkeypatch.setattr(fused, "FORCE", True)


# ------------------------------------------------------------------------------------------------ tests
def test_symbol_is_exported_and_bound():
    from bot_amd import _C
    assert "bot_build_input_reuse_f32" in _C._SIGS and "bot_build_input_reuse_f32" in _C.EXPORTED
    res, args = _C._SIGS["bot_build_input_reuse_f32"]
    assert res is ctypes.c_int and len(args) == 15
    assert hasattr(ctypes.CDLL(_C.LIB_PATH), "bot_build_input_reuse_f32")
    assert callable(_C.build_input_reuse) and isinstance(_C.REUSE_CALLS, int)
    assert _C._lib.bot_abi_version() == 19


def test_argument_refusals_without_gpu():
    """Every refusal happens before a launch: fake non-NULL pointers are never dereferenced on the host."""
    from bot_amd import _C
    f = _C._lib.bot_build_input_reuse_f32
    P = 4096        # any non-NULL value

    def call(feat=P, ldf=7, n=10, F=7, C=5, code=P, reuse=None, pred=P, ldp=5, p=0.0, seed=0, off=None, out=P, ldo=12):
        return f(feat, ldf, n, F, C, code, reuse, pred, ldp, p, seed, off, out, ldo, None)
    assert call(C=129) == -2 and b"C=129" in _C._lib.bot_last_error()
    assert call(C=0) == -2
    assert call(pred=None) == -1 and b"NULL" in _C._lib.bot_last_error()
    assert call(code=None) == -1
    assert call(out=None) == -1
    assert call(feat=None) == -1
    assert call(ldo=11) == -2 and call(ldf=6) == -2 and call(ldp=4) == -2
    assert call(p=1.0) == -2 and call(p=-0.1) == -2
    assert call(n=-1) == -2
    assert call(n=0) == 0                                       # an empty problem is a no-op
    # the wrapper refuses CPU tensors (no fallback) and malformed operands
    feat, code, pred = torch.zeros(4, 3), torch.full((4,), -1, dtype=torch.int32), torch.zeros(4, 2)
    with pytest.raises(_C.BotKernelError):
        _C.build_input_reuse(feat, code, None, pred, 2, 0.0, 0)


def test_reference_restatement():
    """The numpy restatement itself: the three kinds of label block, and the dropout convention of build_input (Philox word c & 3 of block
    n * ceil(W / 4) + c / 4)."""
    rng = np.random.default_rng(0)
    n, F, C = 257, 7, 5
    feat = rng.standard_normal((n, F)).astype(np.float32)
    pred = (3 * rng.standard_normal((n, C))).astype(np.float32)
    code = np.where(rng.random(n) < 0.3, rng.integers(0, C, n), -1).astype(np.int32)
    reuse = (rng.random(n) < 0.8).astype(np.uint8)
    out, keep = reuse_reference(feat, code, reuse, pred, C)
    assert keep.all() and np.array_equal(out[:, :F], feat)
    hot, soft = code >= 0, (code < 0) & (reuse != 0)
    assert np.array_equal(out[hot, F:], np.eye(C, dtype=np.float32)[code[hot]])
    assert not out[~hot & ~soft, F:].any() and (~hot & ~soft).any()
    np.testing.assert_allclose(out[soft, F:].sum(1), 1.0, atol=1e-6)
    np.testing.assert_allclose(out[soft, F:], torch.softmax(torch.from_numpy(pred[soft]).double(), -1).numpy(), atol=1e-7)
    # reuse = None: every node without an input label takes the softmax
    out_all, _ = reuse_reference(feat, code, None, pred, C)
    np.testing.assert_allclose(out_all[~hot, F:].sum(1), 1.0, atol=1e-6)
    # dropout: rate, scaling, one word per element in build_input's order
    a, ka = reuse_reference(feat, code, reuse, pred, C, 0.25, 3)
    b, kb = reuse_reference(feat, code, reuse, pred, C, 0.25, 4)
    assert abs(ka.mean() - 0.75) < 0.02 and not np.array_equal(ka, kb)
    np.testing.assert_allclose(a[ka], (out / np.float32(0.75))[ka], rtol=1e-6)
    assert not a[~ka].any()
    W, nquad = F + C, 3
    w = philox4x32_10(3, np.array([5 * nquad + 2], dtype=np.uint64))[0]
    assert ka[5, 9] == (not (np.float32(w[1] >> 8) * np.float32(1 / 16777216.0) < np.float32(0.25)))
    # the graph-replay offset word moves the stream
    _, kc = reuse_reference(feat, code, reuse, pred, C, 0.25, 3, seed_offset=1)
    assert not np.array_equal(ka, kc)


def _g300_problem(golden):
    import bot_amd
    s, d, n = golden.graph("g300")
    C, fin = 5, 9
    gen = torch.Generator().manual_seed(7)
    feat = torch.randn(n, fin, generator=gen)
    labels = torch.randint(0, C, (n, 1), generator=gen)
    perm = torch.randperm(n, generator=gen)
    return bot_amd.Graph(s, d, n), n, C, fin, feat, labels, perm, gen


@pytest.mark.parametrize("kind,iters,leave_out", [("gat", 1, False), ("gcn", 1, False), ("gat", 2, True)])
def test_new_path_matches_tensor_op_form_on_cpu(golden, reuse_backend, kind, iters, leave_out):
    """`forward_backward(n_label_iters=k)` on the new path (stand-in for the new wrapper, emulated kernels below it) against the tensor-op
    form on the 300-node graph, drop rates 0, fixed mask: loss, pred, every gradient, the BatchNorm buffers; the reuse passes ran without
    autograd and BatchNorm counted 1 + k batches.  `leave_out`: some nodes are in none of train / validation / test."""
    import torch.nn.functional as F
    from bot_amd import _C, nn as bnn, train as T
    from tests.parity_cases import fwd_close, grad_close
    g, n, C, fin, feat, labels, perm, gen = _g300_problem(golden)
    tr, va = perm[: n // 2], perm[n // 2: 3 * n // 4]
    te = perm[3 * n // 4: n - 20] if leave_out else perm[3 * n // 4:]
    mask = torch.rand(tr.shape, generator=gen) < 0.5

    def make():
        torch.manual_seed(3)
        if kind == "gat":
            return bnn.GAT(dim_node=fin + C, dim_edge=0, dim_output=C, n_hidden=16, n_layers=3, n_heads=3, activation=F.relu, norm="batch",
                           linear=True).train()
        return bnn.GCN(in_feats=fin + C, n_classes=C, n_hidden=16, n_layers=3, activation=F.relu, norm="batch", norm_adj="symm",
                       use_linear=True).train()
    kw = dict(use_labels=True, n_label_iters=iters, loss="loge", n_classes=C, mask=mask)
    ref = make()
    T.FUSED_STEP = False
    try:
        loss_ref, pred_ref, _ = T.forward_backward(ref, g, feat, labels, tr, va, te, **kw)
    finally:
        T.FUSED_STEP = True
    model = make()
    c0 = CALLS[0]
    T.DEBUG_KEEP_PREDS, T.DEBUG_PREDS[:] = True, []
    try:
        loss, pred, wn = T.forward_backward(model, g, feat, labels, tr, va, te, **kw)
        kept = list(T.DEBUG_PREDS)
    finally:
        T.DEBUG_KEEP_PREDS, T.DEBUG_PREDS[:] = False, []
    assert CALLS[0] - c0 == iters                                               # the path was taken
    assert len(kept) == iters and not any(t.requires_grad for t in kept)        # ... and the reuse passes carry no autograd graph
    assert pred.requires_grad and wn.shape == (n,)
    assert abs(float(loss) - float(loss_ref)) <= 2e-6 * max(1.0, abs(float(loss_ref)))
    fwd_close(pred, pred_ref.detach().numpy())
    for (k, p), (_, q) in zip(model.named_parameters(), ref.named_parameters()):
        grad_close(p.grad, q.grad.numpy())
    nb = 0
    for (k, b), (_, c) in zip(model.named_buffers(), ref.named_buffers()):
        if k.endswith("num_batches_tracked"):
            assert int(b) == int(c) == 1 + iters, k
            nb += 1
        else:
            np.testing.assert_allclose(b.numpy(), c.numpy(), rtol=1e-6, atol=0, err_msg=k)
    assert nb >= 1
    if leave_out:       # the label columns of a node in none of the sets stay zero: its membership byte is 0
        m = T._reuse_members(n, tr, va, te)
        assert m is not None and int(m.sum()) == n - 20 and not m[perm[n - 20:]].any()
    else:
        assert T._reuse_members(n, tr, va, te) is None                          # the three sets cover every node: NULL


def test_switches_select_the_tensor_op_form(golden, reuse_backend, monkeypatch):
    """FUSED_REUSE = False (BOT_FUSED_REUSE=0), FUSED_STEP = False (BOT_FUSED_STEP=0), CPU tensors without the test switch, more than 128
    classes: label reuse takes the tensor-op form; n_label_iters = 0 never touches the new wrapper."""
    import torch.nn.functional as F
    from bot_amd import nn as bnn, train as T
    g, n, C, fin, feat, labels, perm, gen = _g300_problem(golden)
    tr, va, te = perm[: n // 2], perm[n // 2: 3 * n // 4], perm[3 * n // 4:]
    mask = torch.rand(tr.shape, generator=gen) < 0.5

    def run(iters):
        torch.manual_seed(3)
        model = bnn.GCN(in_feats=fin + C, n_classes=C, n_hidden=8, n_layers=2, activation=F.relu, norm="batch").train()
        c0 = CALLS[0]
        T.forward_backward(model, g, feat, labels, tr, va, te, use_labels=True, n_label_iters=iters, loss="logit", n_classes=C, mask=mask)
        return CALLS[0] - c0
    assert run(1) == 1 and run(0) == 0
    for name in ("FUSED_REUSE", "FUSED_STEP", "FORCE_REUSE"):
        monkeypatch.setattr(T, name, False)
        assert run(1) == 0, name
        monkeypatch.setattr(T, name, True)
    assert not T.reuse_path_ok(feat, 129) and T.reuse_path_ok(feat, 128)


def test_membership_is_cached_per_index_tensors():
    from bot_amd import train as T
    n = 50
    tr, va, te = torch.arange(0, 20), torch.arange(20, 30), torch.arange(30, 45)
    m = T._reuse_members(n, tr, va, te)
    assert m.dtype == torch.uint8 and int(m.sum()) == 45 and T._reuse_members(n, tr, va, te) is m
    te2 = te.clone()
    assert T._reuse_members(n, tr, va, te2) is not m                            # another tensor: another entry
    te.add_(5)                                                                  # modified in place: rebuilt
    m2 = T._reuse_members(n, tr, va, te)
    assert m2 is not m and int(m2.sum()) == 45 and not m2[30:35].any()
    k = len(T._REUSE)
    del te2
    import gc
    gc.collect()
    assert len(T._REUSE) == k - 1                                               # dropped with its tensor


def test_workload_keyword(reuse_backend):
    """workloads.build(..., n_label_iters=k) hands the keyword to the arxiv step; the default leaves the step as it was."""
    from bot_amd import workloads
    wl = workloads.build("arxiv", "cpu", scale=0.004, drop=False, n_label_iters=1)
    c0 = CALLS[0]
    loss, _ = wl.step()
    assert CALLS[0] - c0 == 1 and np.isfinite(float(loss))
    wl0 = workloads.build("arxiv", "cpu", scale=0.004, drop=False)
    c0 = CALLS[0]
    loss0, _ = wl0.step()
    assert CALLS[0] == c0 and np.isfinite(float(loss0))
