"""The deferred `d h` (bot_amd.gemm.DeferredDh, include/bot_gnn.h "d h recomputed in the apply") without a GPU: the emulated backend does
not get the path (deferral needs tensors on the device), a deferred record claimed with another tensor is an error, and the new entry
points are part of the ABI at its unchanged version."""
import os

import pytest
import torch
import torch.nn.functional as F

import bot_amd
from bot_amd import _C, gemm
from bot_amd import nn as bnn
from bot_amd.nn import fused
from tests import _oracle_backend, parity_cases as PC

NEW = ("bot_gemm_halves3_nt_bn_reduce_f32", "bot_gemm_halves3_nt_bn_apply_f32", "bot_gemm_halves3_nt_bn_deferred_max_k")


@pytest.fixture()
def cpu_backend(monkeypatch):
    _oracle_backend.install(monkeypatch)


def test_emulated_backend_keeps_the_storing_form(golden, cpu_backend, monkeypatch):
    """On CPU tensors nothing is deferred, whatever the switch says: the counter stays, the by-product is still claimed, and the gradients
    of a train step are the same bits with the switch on and off."""
    monkeypatch.setattr(fused, "FORCE", True)
    monkeypatch.setattr(gemm, "FORCE", True)
    g = PC.make_graph(golden, "g300", "cpu")
    n = g.number_of_nodes()
    cfg = dict(n_layers=3, n_heads=3, n_hidden=64, norm="batch", non_interactive_attn=False, use_symmetric_norm=False, linear=True, residual=False)
    torch.manual_seed(23)
    model = bnn.GAT(dim_node=24, dim_edge=0, dim_output=5, activation=F.relu, **cfg).train()
    gen = torch.Generator().manual_seed(24)
    feat, gout = torch.randn(n, 24, generator=gen), torch.randn(n, 5, generator=gen)
    grads = []
    for on in (True, False):
        monkeypatch.setattr(gemm, "DH_DEFERRED", on)
        c0, b0, h0 = gemm.DH_DEFERRED_CALLS, gemm.BN_BYPRODUCT_CALLS, fused.HANDLES
        model.zero_grad(set_to_none=True)
        (model(g, feat) * gout).sum().backward()
        assert gemm.DH_DEFERRED_CALLS == c0 and gemm.BN_BYPRODUCT_CALLS - b0 == 2 and fused.HANDLES - h0 == 2
        grads.append({k: v.grad.clone() for k, v in model.named_parameters()})
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), k


def test_a_deferred_record_with_another_tensor_raises():
    """The gradient that was delivered deferred was never written: anything else arriving at the epilogue is an error, never data."""
    x = torch.zeros(4, 6)
    link = gemm.BnLink(x, torch.zeros(6), torch.ones(6), None, None, 0.0, 0)
    handle = gemm.make_handle(x, 4, 6)
    rec = gemm.DeferredDh("stats", None, None, 0, 64, None)
    link.deliver("stats", handle, rec)
    assert link.pending(handle) is rec                      # the delivered tensor: recognised, not consumed
    assert link.claim(handle) == "stats" and link.deferred is None and link.pending(handle) is None
    for arrive in (lambda: torch.zeros(4, 6), lambda: gemm.make_handle(x, 4, 6)):
        for method in ("pending", "stored", "claim"):
            link.deliver("stats", handle, rec)
            other = arrive()
            with pytest.raises(RuntimeError, match="deferred gradient"):
                getattr(link, method)(other)
            assert link.stats is None and link.deferred is None        # nothing stale is left for a later claim
    # without a deferred record a foreign tensor is simply not claimed (the reduce pass runs), as before
    link.deliver("stats", handle)
    assert link.claim(torch.zeros(4, 6)) is None


def test_abi_version_and_new_entry_points():
    assert _C._lib.bot_abi_version() == 19
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bot_gnn.h")).read()
    assert "#define BOT_ABI_VERSION 19" in header
    for name in NEW:
        assert name in _C.EXPORTED and name in _C._SIGS and hasattr(_C._lib, name), name
        assert name + "(" in header, name
    assert _C.dh_deferred_max_k() == 256
    assert bot_amd.gemm.DH_DEFERRED in (True, False)
