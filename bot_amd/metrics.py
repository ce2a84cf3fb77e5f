"""On-device evaluation metrics: OGB's node-property `Evaluator` ("rocauc" for ogbn-proteins, "acc" for ogbn-products / ogbn-arxiv)
without OGB or scikit-learn, and without moving the prediction matrix to the host.

ROC-AUC with ties is a Mann-Whitney count: for every (group, task) `rocauc_counts` returns the integers (n_pos, n_neg, 2U), 2U = the
sum over (positive p, negative q) pairs of 2 [s_q < s_p] + [s_q == s_p], and ROC-AUC = 2U / (2 n_pos n_neg).  Groups (the train /
validation / test split) share one sort.  impl="kernel": `bot_rocauc_f32` (csrc/rocauc.hip); impl="tensor": the same contract in
tensor ops (`torch.sort` per column, tie runs by comparison of neighbours, `cumsum`) - what runs on CPU tensors, and what the kernels
are timed against on the GPU.  Default: the kernel for GPU tensors (BOT_ROCAUC=tensor switches it), the tensor form for CPU tensors."""
from __future__ import annotations

import os

import torch

__all__ = ["rocauc_counts", "rocauc", "accuracy", "Evaluator", "label_codes"]

MAX_GROUPS = 8
NO_POSITIVE = "No positively labeled data available. Cannot compute ROC-AUC."


def label_codes(labels) -> torch.Tensor:
    """int8 codes of a label matrix (int64 / int8 / bool / float): 1 = positive, 0 = negative, -1 = not labelled (a float NaN, as OGB
    has it, or any other value)."""
    if labels.dtype == torch.bool:
        return labels.to(torch.int8)
    one, zero, none = (torch.tensor(v, dtype=torch.int8, device=labels.device) for v in (1, 0, -1))
    return torch.where(labels == 1, one, torch.where(labels == 0, zero, none))


def _check_inputs(pred, labels, groups, n_groups):
    if pred.dim() != 2 or labels.dim() != 2 or pred.shape != labels.shape:
        raise RuntimeError(f"pred and labels must be [n, T] of one shape, got {tuple(pred.shape)} and {tuple(labels.shape)}")
    G = int(n_groups)
    if not 1 <= G <= MAX_GROUPS:
        raise ValueError(f"n_groups={G}: 1 <= n_groups <= {MAX_GROUPS}")
    if groups is not None:
        if groups.dim() != 1 or groups.numel() != pred.shape[0]:
            raise RuntimeError(f"groups must be [{pred.shape[0]}], got {tuple(groups.shape)}")
        if groups.dtype != torch.int8:
            groups = groups.clamp(-1, G).to(torch.int8)          # anything outside [0, G) excludes the row
        groups = groups.contiguous()
    return groups, G


def _order_keys(pred):
    """int32 keys whose signed order is the IEEE order of float32 `pred` (-0.0 folded onto +0.0; denormals kept apart; no float
    comparison anywhere), and the mask of NaNs."""
    b = pred.contiguous().view(torch.int32)
    nan = (b & 0x7FFFFFFF) > 0x7F800000
    b = torch.where(b == -(1 << 31), torch.zeros_like(b), b)
    return torch.where(b < 0, b ^ 0x7FFFFFFF, b), nan


def _counts_tensor(pred, codes, groups, G):
    n, T = pred.shape
    dev = pred.device
    out = torch.zeros((G, T, 3), dtype=torch.int64, device=dev)
    if n == 0:
        return out, torch.zeros(1, dtype=torch.int64, device=dev)
    keys, nan = _order_keys(pred)
    g = torch.zeros(n, dtype=torch.int64, device=dev) if groups is None else groups.to(torch.int64)
    row_ok = (g >= 0) & (g < G)
    counted = row_ok[:, None] & (codes >= 0)
    nan_count = (counted & nan).sum().reshape(1)
    combo = torch.where(counted & ~nan, 2 * g[:, None] + codes.to(torch.int64), torch.full((), -1, dtype=torch.int64, device=dev))
    ks, idx = torch.sort(keys, dim=0)
    combo = combo.gather(0, idx)
    edge = torch.ones((1, T), dtype=torch.bool, device=dev)
    start = torch.cat([edge, ks[1:] != ks[:-1]], 0)              # first entry of a tie run
    end = torch.cat([ks[1:] != ks[:-1], edge], 0)                # last entry of a tie run
    big = torch.full((), n + 1, dtype=torch.int64, device=dev)
    for k in range(G):
        neg = (combo == 2 * k).to(torch.int64)
        pos = (combo == 2 * k + 1).to(torch.int64)
        through = torch.cumsum(neg, 0)                           # negatives of the group in sorted positions [0, j]
        below = through - neg
        # both are non-decreasing along a column: the value at the run's first entry is a running maximum over the starts, the
        # value at its last entry a running minimum over the ends from the other side
        at_start = torch.cummax(torch.where(start, below, torch.zeros_like(below)), 0).values
        at_end = torch.cummin(torch.where(end, through, big).flip(0), 0).values.flip(0)
        out[k, :, 0] = pos.sum(0)
        out[k, :, 1] = neg.sum(0)
        out[k, :, 2] = (pos * (at_start + at_end)).sum(0)
    return out, nan_count


def default_impl(pred) -> str:
    if not pred.is_cuda:
        return "tensor"
    return "tensor" if os.environ.get("BOT_ROCAUC", "").lower() == "tensor" else "kernel"


def rocauc_counts(pred, labels, groups=None, n_groups=1, impl=None, with_nan=False):
    """int64 [G, T, 3] on the device of `pred`: (n_pos, n_neg, 2U) of every (group, task); no host read.
    pred: float32 [n, T] scores (any row stride).  labels: [n, T] int64 / int8 / bool, or float with NaN = not labelled.
    groups: [n] integers, g in [0, n_groups) = the row's group, anything else excludes the row; None = one group of all rows.
    NaN scores of counted entries are left out of the counts; `with_nan=True` also returns their number, int64 [1] on the device
    (`Evaluator` raises on it)."""
    groups, G = _check_inputs(pred, labels, groups, n_groups)
    if pred.dtype != torch.float32:
        pred = pred.to(torch.float32)
    codes = label_codes(labels)
    impl = default_impl(pred) if impl is None else impl
    if impl == "kernel":
        from . import _C
        out, nan_count = _C.rocauc_counts(pred, codes, groups, G)
    elif impl == "tensor":
        out, nan_count = _counts_tensor(pred, codes, groups, G)
    else:
        raise ValueError(f"impl={impl!r}: 'kernel' or 'tensor'")
    return (out, nan_count) if with_nan else out


def _mean_auc(counts):
    p, q, u2 = (counts[..., i].to(torch.float64) for i in range(3))
    ok = (p > 0) & (q > 0)
    auc = torch.where(ok, u2 / (2.0 * p * q).clamp_min(1.0), torch.zeros_like(u2))
    return auc.sum(-1) / ok.sum(-1).to(torch.float64)            # 0 / 0 = NaN: no task of the group qualifies


def rocauc(pred, labels, groups=None, n_groups=1, impl=None):
    """float64 [G] on the device: per group the mean, over the tasks with at least one positive and one negative in that group, of
    2U / (2 n_pos n_neg); NaN where no task qualifies.  No host read."""
    return _mean_auc(rocauc_counts(pred, labels, groups, n_groups, impl))


def accuracy(pred_or_classes, labels, groups=None, n_groups=1):
    """OGB's "acc", float64 [G] on the device: per group the mean over the label columns of the share of labelled rows whose
    predicted class equals the label.  `pred_or_classes`: predicted classes of the labels' shape, or scores [n, C] for one label
    column, taken through argmax.  Plain tensor ops."""
    if labels.dim() != 2 or pred_or_classes.dim() != 2 or labels.shape[0] != pred_or_classes.shape[0]:
        raise RuntimeError(f"predictions and labels must be 2-d over the same rows, got {tuple(pred_or_classes.shape)} and {tuple(labels.shape)}")
    cls = pred_or_classes
    if cls.shape[1] != labels.shape[1]:
        if labels.shape[1] != 1:
            raise RuntimeError(f"scores {tuple(cls.shape)} go with one label column, got {tuple(labels.shape)}")
        cls = cls.argmax(dim=-1, keepdim=True)
    groups, G = _check_inputs(cls, labels, groups, n_groups)
    labelled = labels == labels                                   # a float NaN is "not labelled"
    hit = (labels == cls) & labelled
    g = torch.zeros(labels.shape[0], dtype=torch.int64, device=labels.device) if groups is None else groups.to(torch.int64)
    out = []
    for k in range(G):
        rows = (g == k)[:, None]
        per_task = (hit & rows).sum(0).to(torch.float64) / (labelled & rows).sum(0).to(torch.float64)
        out.append(per_task.mean())
    return torch.stack(out)


_METRICS = {"ogbn-proteins": "rocauc", "ogbn-products": "acc", "ogbn-arxiv": "acc"}


def _as_tensor(x, name):
    if isinstance(x, torch.Tensor):
        return x.detach()
    try:
        import numpy as np
        if isinstance(x, np.ndarray):
            return torch.from_numpy(x)
    except ImportError:
        pass
    raise RuntimeError(f"Arguments to Evaluator need to be either numpy ndarray or torch tensor ({name})")


class Evaluator:
    """`ogb.nodeproppred.Evaluator` for the three node datasets of the reference: `eval({"y_pred": ..., "y_true": ...})` returns
    {"rocauc": float} ("ogbn-proteins") or {"acc": float} ("ogbn-products", "ogbn-arxiv").  Torch tensors of either device or numpy
    arrays; the metric is computed where `y_pred` lives and one value is read back."""

    def __init__(self, name):
        if name not in _METRICS:
            raise ValueError(f"Evaluator serves {tuple(_METRICS)}, not {name!r}")
        self.name = name
        self.eval_metric = _METRICS[name]
        self.num_tasks = 112 if name == "ogbn-proteins" else 1

    def _parse(self, d):
        if "y_true" not in d:
            raise RuntimeError("Missing key of y_true")
        if "y_pred" not in d:
            raise RuntimeError("Missing key of y_pred")
        y_true, y_pred = _as_tensor(d["y_true"], "y_true"), _as_tensor(d["y_pred"], "y_pred")
        if y_true.dim() != 2 or y_pred.dim() != 2:
            raise RuntimeError(f"y_true and y_pred must to 2-dim arrray, {y_true.dim()}-dim array given")
        return y_true.to(y_pred.device), y_pred

    def eval_groups(self, y_pred, y_true, groups=None, n_groups=1):
        """The metric of every group from one call (one sort for "rocauc"): a list of `n_groups` floats.  One host read."""
        y_true, y_pred = self._parse({"y_true": y_true, "y_pred": y_pred})
        if groups is not None:
            groups = _as_tensor(groups, "groups").to(y_pred.device)
        if self.eval_metric == "acc":
            if y_true.shape[0] != y_pred.shape[0] or (y_pred.shape[1] != y_true.shape[1] and y_true.shape[1] != 1):
                raise RuntimeError(f"Shape of y_true and y_pred must be the same, got {tuple(y_true.shape)} and {tuple(y_pred.shape)}")
            return [float(v) for v in accuracy(y_pred, y_true, groups, n_groups).tolist()]
        if y_true.shape != y_pred.shape:
            raise RuntimeError(f"Shape of y_true and y_pred must be the same, got {tuple(y_true.shape)} and {tuple(y_pred.shape)}")
        counts, nan_count = rocauc_counts(y_pred, y_true, groups, n_groups, with_nan=True)
        host = torch.cat([_mean_auc(counts), nan_count.to(torch.float64)]).tolist()      # the one device->host read
        if host[-1] > 0:
            raise ValueError("Input contains NaN.")
        if any(v != v for v in host[:-1]):
            raise RuntimeError(NO_POSITIVE)
        return host[:-1]

    def eval(self, input_dict):
        y_true, y_pred = self._parse(input_dict)
        return {self.eval_metric: self.eval_groups(y_pred, y_true)[0]}

    @property
    def expected_input_format(self):
        shape = "(num_nodes, num_tasks)" if self.eval_metric == "rocauc" else "(num_nodes, 1)"
        return f"input_dict = {{'y_true': y_true, 'y_pred': y_pred}}: torch tensors or numpy arrays of shape {shape}"

    @property
    def expected_output_format(self):
        return f"{{'{self.eval_metric}': float}}"
