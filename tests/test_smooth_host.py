"""Label propagation and Correct and Smooth without a GPU: the float64 restatement (tests/smooth_cases.py) against an independent
dense-matrix formulation, the CPU tensor form of bot_amd/smoothing.py against the restatement, the one-hot / mask / post-step rules,
the error cases, the exported symbol's argument checks, and that C&S does what it is for on a planted-community graph."""
import ctypes
import math

import pytest
import torch

import bot_amd
from bot_amd import _C, smoothing
from tests import smooth_cases as SC

# The project's logit criterion (absolute; the values here lie in [-1, 2]).  The fp32 tensor form on the CPU measured at most 2.0e-6 from
# float64 on graphs of 3 000 and 20 000 nodes.
TOL = 1.0e-5
ALPHAS = (0.5, 0.8, 0.979)


def _graph(name):
    src, dst, n = SC.graph(name)
    return bot_amd.Graph(src, dst, n), src, dst, n


# ------------------------------------------------------------------------------------------------ restatement against dense matrices
@pytest.mark.parametrize("adj", ["DAD", "DA", "AD"])
@pytest.mark.parametrize("n,e", [(1, 0), (17, 40), (300, 1500)])
def test_restatement_agrees_with_dense_matrices(adj, n, e):
    src, dst = SC.powerlaw_graph(n, e, 7 + n, n_isolated=2)
    P = SC.dense_P(src, dst, n, adj)
    gen = torch.Generator().manual_seed(n)
    y0 = torch.randn(n, 5, generator=gen, dtype=torch.float64)
    fixed = torch.randperm(n, generator=gen)[: max(1, n // 4)]
    for alpha in ALPHAS:
        for post, (lo, hi) in SC.POSTS.items():
            got = SC.propagate(src, dst, n, y0, 20, alpha, adj, post)
            assert (got - SC.dense_propagate(P, y0, 20, alpha, lo, hi)).abs().max() <= 1e-12
        got = SC.propagate(src, dst, n, y0, 20, alpha, adj, (fixed, "fix"))
        assert (got - SC.dense_propagate(P, y0, 20, alpha, -math.inf, math.inf, fixed)).abs().max() <= 1e-12
        assert torch.equal(got[fixed], y0[fixed])


def test_restatement_of_correct_and_smooth_against_dense_matrices():
    src, dst, n = SC.graph("tiny")
    y_soft, y_true, mask = SC.cs_inputs("tiny", 7)
    for adj in ("DAD", "DA", "AD"):
        P = SC.dense_P(src, dst, n, adj)
        E = torch.zeros(n, 7, dtype=torch.float64)
        E[mask] = SC.onehot(y_true, 7) - y_soft[mask].double()
        Eh = SC.dense_propagate(P, E, 50, 0.8, -1.0, 1.0)
        s = (E[mask].abs().sum() / mask.numel()) / Eh.abs().sum(1)
        s[torch.isinf(s) | (s > 1000)] = 1.0
        c = y_soft.double() + s[:, None] * Eh
        c = torch.where(torch.isfinite(c), c, y_soft.double())
        got, raw = SC.correct(src, dst, n, y_soft, y_true, mask, adj=adj)
        assert SC.scale_margin(raw) > 0.01
        assert (got - c).abs().max() <= 1e-12
        y = c.clone()
        y[mask] = SC.onehot(y_true, 7)
        assert (SC.smooth(src, dst, n, c, y_true, mask, adj=adj) - SC.dense_propagate(P, y, 50, 0.8, 0.0, 1.0)).abs().max() <= 1e-12
        # without autoscale: the labelled rows of the error are held fixed
        got, _ = SC.correct(src, dst, n, y_soft, y_true, mask, adj=adj, autoscale=False, scale=0.7)
        want = y_soft.double() + 0.7 * SC.dense_propagate(P, E, 50, 0.8, -math.inf, math.inf, mask)
        assert (got - want).abs().max() <= 1e-12


# ------------------------------------------------------------------------------------------------ the CPU tensor form
@pytest.mark.parametrize("autoscale", [True, False])
@pytest.mark.parametrize("alpha", ALPHAS)
@pytest.mark.parametrize("adj", ["DAD", "DA", "AD"])
def test_cpu_tensor_form_against_the_restatement(adj, alpha, autoscale):
    g, src, dst, n = _graph("tiny")
    y_soft, y_true, mask = SC.cs_inputs("tiny", 7)
    ref, raw = SC.correct_and_smooth(src, dst, n, y_soft, y_true, mask, 50, alpha, adj, autoscale)
    assert SC.scale_margin(raw) > 0.01, "a raw autoscale factor lies within 1 % of the threshold: choose another seed"
    cs = smoothing.CorrectAndSmooth(50, alpha, adj, 50, alpha, adj, autoscale=autoscale)
    got = cs(g, y_soft, y_true, mask)
    assert got.dtype == torch.float32 and got.shape == y_soft.shape
    err = (got.double() - ref).abs().max().item()
    print(f"cpu tensor form {adj} alpha={alpha} autoscale={autoscale}: max |diff| = {err:.3e}")
    assert err <= TOL
    # the two stages on their own, and __call__ = smooth(correct(...))
    c = cs.correct(g, y_soft, y_true, mask)
    assert (c.double() - SC.correct(src, dst, n, y_soft, y_true, mask, 50, alpha, adj, autoscale)[0]).abs().max() <= TOL
    assert torch.equal(cs.smooth(g, c, y_true, mask), got)
    assert smoothing.default_impl(y_soft) == "tensor"
    with pytest.raises(_C.BotKernelError):              # the kernel form refuses CPU tensors: no quiet fall-back
        smoothing.CorrectAndSmooth(2, alpha, adj, 2, alpha, adj, impl="kernel")(g, y_soft, y_true, mask)


def test_bool_masks_and_column_labels_give_the_same_result():
    g, src, dst, n = _graph("tiny")
    y_soft, y_true, mask = SC.cs_inputs("tiny", 7)
    order = torch.argsort(mask)                          # a bool mask lists its rows in ascending order
    cs = smoothing.CorrectAndSmooth(10, 0.8, "DA", 10, 0.8, "AD")
    a = cs(g, y_soft, y_true, mask)
    b = cs(g, y_soft, y_true[order].view(-1, 1), SC.member(n, mask))
    assert torch.equal(a, b)


@pytest.mark.parametrize("adj", ["DAD", "DA", "AD"])
def test_label_propagation_rules(adj):
    g, src, dst, n = _graph("tiny")
    labels, ref = SC.lp_reference("tiny", 7, adj)
    _, y_true, mask = SC.cs_inputs("tiny", 7)
    lp = smoothing.LabelPropagation(50, 0.8, adj)
    got = lp(g, labels, mask=mask)
    assert got.shape == (n, 7) and got.dtype == torch.float32                         # one-hot over labels.max() + 1 classes
    assert (got.double() - ref).abs().max() <= TOL
    assert torch.equal(lp(g, labels.view(-1, 1), mask=SC.member(n, mask)), got)       # [N, 1] labels, bool mask
    assert got.min() >= 0 and got.max() <= 1                                          # "clamp01"
    # float labels are taken as they are; rows outside the mask start at zero
    soft = SC.cs_inputs("tiny", 7)[0]
    for post in ("clamp01", "clamp11", None, (mask[:20], "fix")):
        got = lp(g, 3.0 * soft - 1.0, mask=mask, post_step=post)
        want = SC.label_propagation(src, dst, n, 3.0 * soft - 1.0, 50, 0.8, adj, mask=mask, post_step=post)
        assert (got.double() - want).abs().max() <= TOL, post
    start = torch.where(SC.member(n, mask)[:, None], 3.0 * soft - 1.0, torch.zeros(()))
    assert torch.equal(got[mask[:20]], start[mask[:20]])                              # fixed rows keep their start values
    assert torch.equal(smoothing.LabelPropagation(0, 0.8, adj)(g, soft, post_step=None), soft)
    # without a mask every row starts from its label
    want = SC.label_propagation(src, dst, n, labels, 50, 0.8, adj)
    assert (lp(g, labels).double() - want).abs().max() <= TOL


def test_error_cases():
    g, src, dst, n = _graph("tiny")
    y_soft, y_true, mask = SC.cs_inputs("tiny", 7)
    cs = smoothing.CorrectAndSmooth(2, 0.8, "DAD", 2, 0.8, "DAD")
    with pytest.raises(ValueError, match="empty"):
        cs(g, y_soft, y_true[:0], mask[:0])
    with pytest.raises(ValueError, match="empty"):
        cs.correct(g, y_soft, y_true[:0], torch.zeros(n, dtype=torch.bool))
    with pytest.raises(ValueError, match="multi-class"):
        cs(g, y_soft, torch.stack([y_true, y_true], 1), mask)
    with pytest.raises(ValueError, match="multi-class"):
        smoothing.LabelPropagation(2, 0.5)(g, torch.zeros(n, 2, dtype=torch.int64))
    with pytest.raises(ValueError):
        cs(g, y_soft, y_true[:-1], mask)
    with pytest.raises(ValueError):
        smoothing.LabelPropagation(2, 0.5, adj="ADA")
    with pytest.raises(ValueError):
        smoothing.CorrectAndSmooth(smoothing_adj="D")
    with pytest.raises(ValueError):
        smoothing.LabelPropagation(2, 0.5)(g, y_soft, post_step="clamp")
    with pytest.raises(ValueError):
        smoothing.LabelPropagation(2, 0.5, impl="triton")(g, y_soft)
    with pytest.raises(ValueError):
        smoothing.LabelPropagation(2, 0.5)(g, y_soft[:-1])
    block = bot_amd.Graph(src[dst < 100], dst[dst < 100], n, num_dst_nodes=100)       # a block: fewer destinations than sources
    with pytest.raises(ValueError, match="square"):
        cs(block, y_soft, y_true, mask)
    with pytest.raises(ValueError, match="square"):
        smoothing.LabelPropagation(2, 0.5)(block, y_soft)


def test_default_impl_follows_the_environment(monkeypatch):
    class Fake:
        is_cuda = True
    monkeypatch.delenv("BOT_SMOOTH", raising=False)
    assert smoothing.default_impl(Fake()) == "kernel"
    monkeypatch.setenv("BOT_SMOOTH", "tensor")
    assert smoothing.default_impl(Fake()) == "tensor"
    assert smoothing.default_impl(torch.zeros(1)) == "tensor"
    assert bot_amd.CorrectAndSmooth is smoothing.CorrectAndSmooth and bot_amd.LabelPropagation is smoothing.LabelPropagation


# ------------------------------------------------------------------------------------------------ the symbol
def test_propagate_step_symbol_checks_its_arguments_without_a_gpu():
    lib = _C._lib
    assert "bot_propagate_step_f32" in _C.EXPORTED and _C.ABI_VERSION == 19 and lib.bot_abi_version() == 19
    buf = (ctypes.c_float * 64)()
    items = (ctypes.c_int32 * 64)()
    p, p2 = ctypes.addressof(buf), ctypes.addressof(buf) + 128
    it = (ctypes.addressof(items) + 15) // 16 * 16

    def call(y=p, y0=p, out=p2, C=4, n=4, nnz=0, items=it, ld=4, n_long=0):
        return lib.bot_propagate_step_f32(None, None, n, nnz, items, n, None, None, n_long, y, ld, y0, ld, out, ld, C, 0.5, 0.5, None, None,
                                          -math.inf, math.inf, None, None, None, None, None)
    assert call(y=None) == -1 and b"NULL" in lib.bot_last_error()
    assert call(y0=None) == -1 and call(out=None) == -1 and call(items=None) == -1
    assert call(nnz=3) == -1 and b"indices" in lib.bot_last_error()
    assert call(n_long=1) == -1
    assert call(C=0) == -2 and b"C=0" in lib.bot_last_error()
    assert call(C=1025, ld=1025) == -2 and b"C=1025" in lib.bot_last_error()
    assert call(n=-1) == -2 and call(ld=3) == -2
    assert call(out=p) == -2 and b"alias" in lib.bot_last_error()
    assert call(y=None, y0=None, out=None, items=None, n=0) == 0                      # an empty problem


# ------------------------------------------------------------------------------------------------ what it is for
def test_correct_and_smooth_improves_a_noisy_predictor_on_planted_communities():
    """10 % of the labels known, a base predictor that is right about 60 % of the time: on the unlabelled nodes the float64 restatement of
    C&S is strictly more accurate than the base predictor, and the CPU tensor form classifies as the restatement does."""
    n, k = 2000, 5
    src, dst, comm = SC.planted_graph(n, k, 8000, 0.9, seed=1)
    gen = torch.Generator().manual_seed(2)
    y_soft = torch.softmax(1.2 * SC.onehot(comm, k).float() + torch.randn(n, k, generator=gen), dim=-1)
    perm = torch.randperm(n, generator=gen)
    known, rest = perm[: n // 10], perm[n // 10:]
    base = (y_soft[rest].argmax(1) == comm[rest]).double().mean().item()
    for autoscale in (True, False):
        ref, _ = SC.correct_and_smooth(src, dst, n, y_soft, comm[known], known, autoscale=autoscale)
        acc = (ref[rest].argmax(1) == comm[rest]).double().mean().item()
        print(f"planted communities, autoscale={autoscale}: base {base:.3f} -> C&S {acc:.3f}")
        assert 0.4 < base < 0.8 and acc > base
        assert torch.equal(ref[known].argmax(1), comm[known])
    got = smoothing.CorrectAndSmooth(autoscale=False)(bot_amd.Graph(src, dst, n), y_soft, comm[known], known)
    assert (got.double() - ref).abs().max() <= TOL
