"""bot_amd.metrics without a GPU: the numpy restatement (tests/metrics_cases.py) against scikit-learn, the tensor-op form of
`rocauc_counts` against the restatement integer for integer, the means, `accuracy`, the OGB surface of `Evaluator`, the argument
checks of bot_rocauc_f32 (which stop before any launch) and `minibatch.evaluate_scores` on a stub model and loader."""
import ctypes

import numpy as np
import pytest
import torch

from bot_amd import _C, metrics, minibatch
from tests import metrics_cases as MC


def _t(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x))


# ------------------------------------------------------------------------------------------------ 1. the restatement itself
@pytest.mark.parametrize("family", ["continuous", "levels2", "levels7", "levels300", "equal"])
@pytest.mark.parametrize("n", [2, 65, 1000, 5000])
def test_restatement_against_scikit_learn(family, n):
    """|2U / (2 p q) - sklearn.metrics.roc_auc_score| <= 1e-12: scikit-learn sums at most n trapezoids in float64, n 2^-53 = 5.6e-13
    at n = 5 000 (observed on such inputs: 1.1e-16)."""
    sk = pytest.importorskip("sklearn.metrics")
    pred, labels, _ = MC.case(family, n, 4, 1, seed=n, unlabelled=0.0)
    labels[0, :], labels[1, :] = 1, 0                      # both classes in every task, so scikit-learn accepts it
    counts, nans = MC.counts_reference(pred, labels)
    assert nans == 0
    for t in range(4):
        p, q, u2 = (int(v) for v in counts[0, t])
        assert p == int((labels[:, t] == 1).sum()) and q == n - p
        ref = sk.roc_auc_score(labels[:, t], pred[:, t])
        err = abs(u2 / (2.0 * p * q) - ref)
        print(f"{family} n={n} task {t}: |restatement - sklearn| = {err:.3e}")
        assert err <= 1e-12


def test_restatement_on_a_hand_case():
    """Scores 1, 1, 2, 3 with labels 0, 1, 1, 0, by hand: the positive at 1 ties one negative (1) and is below the other (0), the
    positive at 2 is above one negative (2) and below the other (0): 2U = 3."""
    counts, _ = MC.counts_reference(np.array([[1.0], [1.0], [2.0], [3.0]], dtype=np.float32), np.array([[0], [1], [1], [0]]))
    assert counts.tolist() == [[[2, 2, 3]]]


# ------------------------------------------------------------------------------------------------ 2. the tensor-op form
@pytest.mark.parametrize("family", MC.FAMILIES)
@pytest.mark.parametrize("n,T,G", [(1, 1, 1), (2, 3, 3), (64, 1, 1), (65, 3, 3), (1500, 5, 1), (3000, 4, 3)])
def test_tensor_path_equals_the_restatement(family, n, T, G):
    """Groups absent and three groups with excluded rows; a one-class task (task 1 where T >= 3); +-0.0, +-inf, denormals
    ("special"); logits of magnitude 125 ("large"): every one of the G T 3 integers."""
    pred, labels, groups = MC.case(family, n, T, G, seed=7 * n + T)
    ref, nans = MC.counts_reference(pred, labels, groups, G)
    got, nan_count = metrics.rocauc_counts(_t(pred), _t(labels), _t(groups), G, impl="tensor", with_nan=True)
    assert got.dtype == torch.int64 and tuple(got.shape) == (G, T, 3)
    assert np.array_equal(got.numpy(), ref) and int(nan_count) == nans == 0
    assert np.array_equal(metrics.rocauc_counts(_t(pred), _t(labels), _t(groups), G).numpy(), ref)     # the default on CPU tensors


def test_tensor_path_label_types_strides_and_empty_groups():
    pred, labels, groups = MC.case("levels7", 900, 6, 3, seed=3)
    ref, _ = MC.counts_reference(pred, labels, groups, 3)
    p, g = _t(pred), _t(groups)
    as_float = labels.astype(np.float32)
    as_float[labels < 0] = np.nan                          # OGB's "not labelled"
    assert np.array_equal(metrics.rocauc_counts(p, _t(as_float), g, 3, impl="tensor").numpy(), ref)
    assert np.array_equal(metrics.rocauc_counts(p, _t(labels.astype(np.int64)), g.to(torch.int64), 3, impl="tensor").numpy(), ref)
    full = np.abs(labels)                                  # bool labels have no "not labelled"
    ref_b, _ = MC.counts_reference(pred, full, groups, 3)
    assert np.array_equal(metrics.rocauc_counts(p, _t(full.astype(bool)), g, 3, impl="tensor").numpy(), ref_b)
    wide = torch.zeros(900, 11)
    wide[:, 2:8] = p
    assert np.array_equal(metrics.rocauc_counts(wide[:, 2:8], _t(labels), g, 3, impl="tensor").numpy(), ref)     # strided pred
    # an empty group: nobody is in group 1; and G larger than the groups present
    g2 = groups.copy()
    g2[g2 == 1] = -1
    ref_e, _ = MC.counts_reference(pred, labels, g2, 4)
    got = metrics.rocauc_counts(p, _t(labels), _t(g2), 4, impl="tensor").numpy()
    assert np.array_equal(got, ref_e) and not got[1].any() and not got[3].any()
    # task 1 holds positives only: no pair, 2U = 0
    assert (ref[:, 1, 1] == 0).all() and (ref[:, 1, 2] == 0).all() and (ref[:, 1, 0] > 0).all()
    # no rows
    assert not metrics.rocauc_counts(torch.zeros(0, 5), torch.zeros(0, 5, dtype=torch.int8), None, 2, impl="tensor").any()
    with pytest.raises(ValueError):
        metrics.rocauc_counts(p, _t(labels), g, 9)
    with pytest.raises(ValueError):
        metrics.rocauc_counts(p, _t(labels), g, 3, impl="eager")
    with pytest.raises(RuntimeError):
        metrics.rocauc_counts(p[:, :5], _t(labels), g, 3)
    with pytest.raises(_C.BotKernelError):
        metrics.rocauc_counts(p, _t(labels), g, 3, impl="kernel")          # the kernels take GPU tensors only


def test_tensor_path_counts_nans_of_counted_entries_only():
    pred, labels, groups = MC.case("continuous", 500, 3, 3, seed=11)
    counted = np.flatnonzero((groups >= 0) & (labels[:, 0] >= 0))
    skipped_row, unlabelled = np.flatnonzero(groups < 0)[0], np.flatnonzero((labels[:, 2] < 0) & (groups >= 0))[0]
    pred[skipped_row, 0] = np.nan
    pred[unlabelled, 2] = np.nan
    ref, nans = MC.counts_reference(pred, labels, groups, 3)
    got, nan_count = metrics.rocauc_counts(_t(pred), _t(labels), _t(groups), 3, impl="tensor", with_nan=True)
    assert nans == 0 and int(nan_count) == 0 and np.array_equal(got.numpy(), ref)
    pred[counted[:2], 0] = np.nan
    ref, nans = MC.counts_reference(pred, labels, groups, 3)
    got, nan_count = metrics.rocauc_counts(_t(pred), _t(labels), _t(groups), 3, impl="tensor", with_nan=True)
    assert nans == 2 and int(nan_count) == 2 and np.array_equal(got.numpy(), ref)


# ------------------------------------------------------------------------------------------------ 3. means and accuracy
def test_rocauc_mean_and_accuracy():
    """`rocauc` against the restatement's mean within 1e-13 (at most 112 terms, each at most 1, in float64); NaN for a group without
    a qualifying task; `accuracy` against numpy."""
    pred, labels, groups = MC.case("levels300", 2000, 112, 3, seed=5)
    groups[groups == 2] = -1                               # group 2 is empty: NaN
    ref = MC.mean_auc_reference(MC.counts_reference(pred, labels, groups, 3)[0])
    got = metrics.rocauc(_t(pred), _t(labels), _t(groups), 3)
    assert got.dtype == torch.float64 and tuple(got.shape) == (3,)
    assert np.abs(got.numpy()[:2] - ref[:2]).max() <= 1e-13 and np.isnan(ref[2]) and np.isnan(got.numpy()[2])
    rng = np.random.default_rng(0)
    y = rng.integers(0, 47, (3000, 1))
    scores = rng.standard_normal((3000, 47)).astype(np.float32)
    scores[np.arange(3000), y[:, 0]] += 2.0
    cls = scores.argmax(1)[:, None]
    g = rng.integers(-1, 3, 3000).astype(np.int8)
    want = np.array([(cls[g == k] == y[g == k]).mean() for k in range(3)])
    assert np.abs(metrics.accuracy(_t(scores), _t(y), _t(g), 3).numpy() - want).max() <= 1e-15
    assert np.abs(metrics.accuracy(_t(cls), _t(y), _t(g), 3).numpy() - want).max() <= 1e-15
    assert abs(float(metrics.accuracy(_t(cls), _t(y))[0]) - (cls == y).mean()) <= 1e-15


# ------------------------------------------------------------------------------------------------ 4. Evaluator
def test_evaluator_surface_and_errors():
    ev = metrics.Evaluator("ogbn-proteins")
    assert ev.eval_metric == "rocauc" and metrics.Evaluator("ogbn-products").eval_metric == "acc" and metrics.Evaluator("ogbn-arxiv").eval_metric == "acc"
    with pytest.raises(ValueError):
        metrics.Evaluator("ogbn-mag")
    pred, labels, _ = MC.case("levels7", 800, 5, 1, seed=2)
    want = MC.mean_auc_reference(MC.counts_reference(pred, labels)[0])[0]
    for yp, yt in ((pred, labels), (_t(pred), _t(labels)), (_t(pred), _t(labels.astype(np.int64)))):       # numpy and tensors
        out = ev.eval({"y_pred": yp, "y_true": yt})
        assert list(out) == ["rocauc"] and isinstance(out["rocauc"], float) and abs(out["rocauc"] - want) <= 1e-13
    with pytest.raises(RuntimeError, match="No positively labeled data available. Cannot compute ROC-AUC."):
        ev.eval({"y_pred": pred, "y_true": np.ones_like(labels)})
    with pytest.raises(RuntimeError):
        ev.eval({"y_pred": pred[:, :4], "y_true": labels})
    with pytest.raises(RuntimeError):
        ev.eval({"y_pred": pred})
    bad = pred.copy()
    bad[np.flatnonzero(labels[:, 0] >= 0)[0], 0] = np.nan
    with pytest.raises(ValueError):
        ev.eval({"y_pred": bad, "y_true": labels})
    acc = metrics.Evaluator("ogbn-products")
    y = np.arange(10)[:, None] % 3
    out = acc.eval({"y_pred": np.zeros((10, 1), dtype=np.int64), "y_true": y})
    assert list(out) == ["acc"] and abs(out["acc"] - 0.4) <= 1e-15
    with pytest.raises(RuntimeError):
        acc.eval({"y_pred": np.zeros((9, 1), dtype=np.int64), "y_true": y})


def test_the_reference_wrappers_work_as_written():
    """ogbn-proteins/gat.py:175 and ogbn-products/gat.py:197-199, verbatim."""
    pred, labels, _ = MC.case("continuous", 600, 112, 1, seed=9)
    evaluator = metrics.Evaluator("ogbn-proteins")
    evaluator_wrapper = lambda pred, labels: evaluator.eval({"y_pred": pred, "y_true": labels})["rocauc"]
    want = MC.mean_auc_reference(MC.counts_reference(pred, labels)[0])[0]
    assert abs(evaluator_wrapper(_t(pred), _t(labels.astype(np.int64))) - want) <= 1e-13
    evaluator = metrics.Evaluator("ogbn-products")
    evaluator_wrapper = lambda pred, labels: evaluator.eval(
        {"y_pred": pred.argmax(dim=-1, keepdim=True), "y_true": labels}
    )["acc"]
    y = torch.randint(0, 47, (600, 1), generator=torch.Generator().manual_seed(0))
    scores = torch.randn(600, 47, generator=torch.Generator().manual_seed(1))
    assert abs(evaluator_wrapper(scores, y) - float((scores.argmax(1, keepdim=True) == y).double().mean())) <= 1e-15


# ------------------------------------------------------------------------------------------------ 5. the C ABI, no launch
def test_rocauc_argument_checks_without_gpu():
    """Every refusal returns before a launch: ranges (BOT_E_RANGE = -2), NULL pointers (BOT_E_NULL = -1); the workspace size is
    non-decreasing in n, T and G."""
    lib = _C._lib
    buf = (ctypes.c_int64 * 64)()
    p = ctypes.addressof(buf)
    f = lib.bot_rocauc_f32
    big = 1 << 50
    assert f(p, 4, p, 4, None, 1 << 31, 4, 1, p, p, p, big, None) == -2 and b"rocauc" in lib.bot_last_error()
    assert f(p, 4, p, 4, None, -1, 4, 1, p, p, p, big, None) == -2
    assert f(p, 4, p, 4, None, 10, 0, 1, p, p, p, big, None) == -2
    assert f(p, 65536, p, 65536, None, 10, 65536, 1, p, p, p, big, None) == -2
    assert f(p, 1024, p, 1024, None, 1 << 30, 1024, 1, p, p, p, big, None) == -2          # n T = 2^40
    assert f(p, 4, p, 4, None, 10, 4, 0, p, p, p, big, None) == -2
    assert f(p, 4, p, 4, None, 10, 4, 9, p, p, p, big, None) == -2
    assert f(p, 3, p, 4, None, 10, 4, 1, p, p, p, big, None) == -2                        # ldp < T
    assert f(p, 4, p, 3, None, 10, 4, 1, p, p, p, big, None) == -2
    assert f(p, 4, p, 4, None, 10, 4, 1, None, p, p, big, None) == -1
    assert f(p, 4, p, 4, None, 10, 4, 1, p, None, p, big, None) == -1
    assert f(None, 4, p, 4, None, 10, 4, 1, p, p, p, big, None) == -1 and b"NULL" in lib.bot_last_error()
    assert f(p, 4, None, 4, None, 10, 4, 1, p, p, p, big, None) == -1
    assert f(p, 4, p, 4, None, 10, 4, 1, p, p, None, big, None) == -1
    assert f(p, 4, p, 4, None, 10, 4, 1, p, p, p, lib.bot_rocauc_workspace_bytes(10, 4, 1) - 1, None) == -2   # workspace too small
    assert f(None, 4, None, 4, None, 0, 4, 1, p, p, None, 0, None) == 0                   # no rows: nothing launched
    w = lib.bot_rocauc_workspace_bytes
    assert w(1 << 31, 1, 1) == -1 and w(10, 0, 1) == -1 and w(10, 1, 9) == -1 and w(1 << 30, 1024, 1) == -1
    ns, ts = (0, 1, 63, 4096, 4097, 70001, 132534, 1 << 20), (1, 3, 112, 4000)
    for G in (1, 3, 8):
        for a, b in zip(ns, ns[1:]):
            assert all(0 <= w(a, T, G) <= w(b, T, G) for T in ts)
        for a, b in zip(ts, ts[1:]):
            assert all(w(n, a, G) <= w(n, b, G) for n in ns)
    assert all(w(n, T, 1) <= w(n, T, 3) <= w(n, T, 8) for n in ns for T in ts)
    assert w(132534, 112, 3) >= 10 * 132534 * 112


# ------------------------------------------------------------------------------------------------ 6. the evaluation loop
class _Table(torch.nn.Module):
    def __init__(self, table):
        super().__init__()
        self.table = table

    def forward(self, blocks):
        return self.table[blocks]


class _Loader:
    """Yields (input_nodes, output_nodes, blocks) over all nodes in batches of 97; `blocks` is the output ids, which _Table reads."""

    class _G:
        device = torch.device("cpu")

    def __init__(self, n):
        self.g, self.n = self._G(), n

    def __iter__(self):
        for lo in range(0, self.n, 97):
            out = torch.arange(lo, min(self.n, lo + 97))
            yield out, out, out


def test_evaluate_scores_order_and_grouped_call():
    n = 700
    pred, labels, _ = MC.case("levels300", n, 12, 1, seed=4, unlabelled=0.0)
    table, y = _t(pred), _t(labels.astype(np.int64))
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(0))
    tr, va, te = perm[:350], perm[350:480], perm[480:650]                  # 50 nodes are in no split
    crit = lambda x, t: torch.nn.functional.binary_cross_entropy_with_logits(x, t.float())
    ev = metrics.Evaluator("ogbn-proteins")
    out = minibatch.evaluate_scores(_Table(table), _Loader(n), y, tr, va, te, crit, ev)
    assert len(out) == 7 and torch.equal(out[6], table)
    wrapper = lambda p, l: ev.eval({"y_pred": p, "y_true": l})["rocauc"]
    per_split = minibatch.evaluate_scores(_Table(table), _Loader(n), y, tr, va, te, crit, wrapper)
    for k, idx in enumerate((tr, va, te)):
        want = MC.mean_auc_reference(MC.counts_reference(pred[idx.numpy()], labels[idx.numpy()])[0])[0]
        assert abs(out[k] - want) <= 1e-13 and abs(per_split[k] - want) <= 1e-13
        assert out[3 + k] == per_split[3 + k] == float(crit(table[idx], y[idx]))
    # "acc" on scores, eval_times = 2 (the same table twice: the average is the table)
    yc = torch.randint(0, 12, (n, 1), generator=torch.Generator().manual_seed(2))
    acc = minibatch.evaluate_scores(_Table(table), _Loader(n), yc, tr, va, te, lambda x, t: torch.nn.functional.cross_entropy(x, t[:, 0]),
                                    metrics.Evaluator("ogbn-products"), eval_times=2, n_classes=12)
    for k, idx in enumerate((tr, va, te)):
        assert abs(acc[k] - float((table[idx].argmax(1, keepdim=True) == yc[idx]).double().mean())) <= 1e-15


def test_build_sampled_takes_the_evaluation_defaults_lazily():
    import inspect

    from bot_amd import workloads
    sig = inspect.signature(workloads.build_sampled).parameters
    assert sig["eval_fanouts"].default is None and sig["eval_batch_size"].default is None
    fan, batch = workloads.SAMPLED_EVAL["proteins"]
    assert fan == 100 and batch(132534) == 65536
    fan, batch = workloads.SAMPLED_EVAL["products"]
    assert fan == 8 and batch(2449029) == -(-2449029 // 30)
    assert isinstance(workloads.SampledWorkload.eval_loader, property)
