"""Post-processing of a model's predictions on the graph: label propagation (`LabelPropagation`, DGL's `dgl.nn.LabelPropagation`)
and Correct and Smooth (`CorrectAndSmooth`; Huang et al., ICLR 2021, DGL's `correct_and_smooth` example).

Both iterate  y <- post(alpha * P y + (1 - alpha) * y_start)  with P a degree-normalised adjacency: with
deg = in_degrees().float().clamp(min=1) and (A y)[v] = the sum of y[u] over the in-edges u -> v (`ops.copy_u_sum`), P is
D^-1/2 A D^-1/2 ("DAD"), D^-1 A ("DA") or A D^-1 ("AD").  Rows are in the graph's own node numbering, as for every op of
`bot_amd.ops`.  impl="kernel": one `bot_propagate_step_f32` launch per iteration on two ping-pong buffers (csrc/propagate.hip: the row
scale, the axpy, the clamp, the reset of fixed rows and the row norms are the gather's epilogue); impl="tensor": the same contract in
tensor ops - on the GPU `_C.spmm` with the normalisation as position-order edge weights and (1 - alpha) * y_start as addend, then torch
ops; on a CPU-resident graph `index_add_` - what runs on CPU tensors, and what the kernel is timed against.  Default: see `default_impl`.

Edge weights (`edge_weight=`: a float32 [E] / [E, 1] tensor in edge-id order, or an `edata` key): (A y)[v] becomes the sum of
w_e * y[u] and the degree vector of all three normalisations the WEIGHTED in-degree, deg[v] = s[v] if s[v] > 0 else 1 with
s[v] = the float32 sum of w_e over the in-edges of v (unit weights: today's deg, bit for bit).  impl="kernel" streams the weights in CSC
position order beside the ids (`bot_propagate_step_w_f32`); impl="tensor" multiplies them into the SpMM's edge weights / the gathered
rows.  Weights are expected finite and non-negative and are not checked - a check would be a host read.

Limits: one GPU, multi-class labels (one label column), square graphs only (whole graphs and `Subgraph`s; a block or a
partition with a halo raises)."""
from __future__ import annotations

import math
import os

import torch

__all__ = ["LabelPropagation", "CorrectAndSmooth", "evaluate_smoothed", "default_impl", "propagate"]

_ADJ = ("DAD", "DA", "AD")
_INF = math.inf


# The weighted kernel form is the default with a weight only while it beats the weighted tensor form by more than that form's
# round-to-round spread (tools/bench_smooth.py --edge-weight); the measurement sets this flag.
WEIGHTED_KERNEL = True


def default_impl(x, weighted=False) -> str:
    """"kernel" for GPU tensors unless BOT_SMOOTH=tensor, "tensor" for CPU tensors; `weighted`: a run with edge weights (the kernel form
    while `WEIGHTED_KERNEL` holds)."""
    if not x.is_cuda:
        return "tensor"
    if weighted and not WEIGHTED_KERNEL:
        return "tensor"
    return "tensor" if os.environ.get("BOT_SMOOTH", "").lower() == "tensor" else "kernel"


def _square(g):
    if g.is_block or g.halo is not None:
        raise ValueError("label propagation takes a square graph (a whole graph or a Subgraph), not a block or a partition with a halo")


def _cache(g):
    c = getattr(g, "_bot_smooth", None)
    if c is None:
        c = g._bot_smooth = {}
    return c


def _weights(g, edge_weight):
    """The per-graph state of a run with edge weights, or None without: a dict that holds "eid" (float32 [E], edge-id order), "pos"
    (the contiguous CSC-position copy the kernel and the SpMM stream) and, filled on demand, the weighted degree scales ("deg") and the
    tensor form's products (("w", adj)).  One weight at a time is kept per graph, under the tensor's identity and `_version`: an
    in-place change prepares everything again."""
    if edge_weight is None:
        return None
    w = g.edata[edge_weight] if isinstance(edge_weight, str) else edge_weight
    if not isinstance(w, torch.Tensor):
        raise TypeError(f"edge_weight must be an edata key or a tensor, got {type(edge_weight).__name__}")
    E = g.number_of_edges()
    if w.shape not in ((E,), (E, 1)) or w.dtype != torch.float32:
        raise ValueError(f"edge_weight must be float32 [{E}] or [{E}, 1], got {tuple(w.shape)} {w.dtype}")
    if w.device != g.device:
        raise ValueError(f"edge_weight lives on {w.device}, the graph on {g.device}")
    c = _cache(g)
    hit = c.get("ew")
    if hit is not None and hit[0] is w and hit[1] == w._version:
        return hit[2]
    c["ew"] = None                                   # drop the old copies before allocating the new ones
    flat = w.detach().reshape(E)
    ws = {"eid": flat, "pos": flat[g.csc.eid.long()].contiguous()}
    c["ew"] = (w, w._version, ws)
    return ws


def _degree_scales(g, adj, ws=None):
    """(src_scale, dst_scale): float32 [N] or None, cached per graph (with weights `ws`: beside them, from the weighted in-degree).
    P y = dst_scale * A (src_scale * y)."""
    if ws is not None:
        if "deg" not in ws:
            if g.device.type == "cuda":
                from . import _C
                s = _C.segment_sum(g.csc, ws["pos"].view(-1, 1)).view(-1)
            else:
                s = torch.zeros(g.number_of_nodes(), dtype=torch.float32).index_add_(0, g.edges()[1], ws["eid"])
            d = torch.where(s > 0, s, torch.ones((), dtype=torch.float32, device=s.device))
            ws["deg"] = (torch.pow(d, -0.5).contiguous(), (1.0 / d).contiguous())
        rsqrt, inv = ws["deg"]
        return {"DAD": (rsqrt, rsqrt), "DA": (None, inv), "AD": (inv, None)}[adj]
    c = _cache(g)
    if "deg" not in c:
        if g.device.type == "cuda":
            deg = g.in_degrees()
        else:
            deg = torch.bincount(g.edges()[1], minlength=g.number_of_nodes())
        d = deg.float().clamp(min=1)
        c["deg"] = (torch.pow(d, -0.5).contiguous(), (1.0 / d).contiguous())
    rsqrt, inv = c["deg"]
    return {"DAD": (rsqrt, rsqrt), "DA": (None, inv), "AD": (inv, None)}[adj]


def _edge_weights(g, adj, ws=None):
    """float32 [E, 1] in CSC position order: dst_scale[row of k] * src_scale[indices[k]] (the tensor form's SpMM weights), cached; with
    weights `ws` times ws["pos"][k], cached beside them."""
    c = _cache(g) if ws is None else ws
    if ("w", adj) not in c:
        src_scale, dst_scale = _degree_scales(g, adj, ws)
        d = g.csc
        w = torch.ones(d.nnz, dtype=torch.float32, device=d.indices.device) if ws is None else ws["pos"]
        if src_scale is not None:
            w = w * src_scale[d.indices.long()]
        if dst_scale is not None:
            rows = torch.repeat_interleave(torch.arange(d.n_rows, device=w.device), (d.indptr[1:] - d.indptr[:-1]).long(), output_size=d.nnz)
            w = w * dst_scale[rows]
        c[("w", adj)] = w.view(-1, 1).contiguous()
    return c[("w", adj)]


def _member(n, mask, device):
    """bool [N]: the rows of `mask` (an index tensor or a bool [N]); no host read."""
    mask = torch.as_tensor(mask, device=device)
    if mask.dtype == torch.bool:
        if mask.shape != (n,):
            raise ValueError(f"a bool mask must be [{n}], got {tuple(mask.shape)}")
        return mask
    return torch.zeros(n, dtype=torch.bool, device=device).index_fill_(0, mask.long(), True)      # (m[idx] = True synchronises)


def _rows_to_full(n, mask, values):
    """[N, C] with the rows of `mask` (index or bool [N]) set to `values` (one row per masked node, in mask order) and zeros elsewhere;
    no host read (a bool mask is resolved with a cumsum, not with nonzero)."""
    mask = torch.as_tensor(mask, device=values.device)
    if mask.dtype == torch.bool:
        pos = (torch.cumsum(mask.long(), 0) - 1).clamp_(min=0, max=max(values.shape[0] - 1, 0))
        return torch.where(mask[:, None], values[pos], torch.zeros((), dtype=values.dtype, device=values.device))
    full = torch.zeros((n, values.shape[1]), dtype=values.dtype, device=values.device)
    return full.index_copy_(0, mask.long(), values)


def _onehot(y, C, dtype, device):
    y = torch.as_tensor(y, device=device)
    if y.dim() == 2:
        if y.shape[1] != 1:
            raise ValueError(f"labels must be [n] or [n, 1] class ids (multi-class only), got {tuple(y.shape)}")
        y = y[:, 0]
    if y.dim() != 1:
        raise ValueError(f"labels must be [n] or [n, 1] class ids, got {tuple(y.shape)}")
    out = torch.zeros((y.shape[0], C), dtype=dtype, device=device)
    return out.scatter_(1, y.long().view(-1, 1), 1.0)


def _post(post_step, n, device):
    """post_step -> (lo, hi, fixed bool [N] or None)."""
    if post_step is None:
        return -_INF, _INF, None
    if post_step == "clamp01":
        return 0.0, 1.0, None
    if post_step == "clamp11":
        return -1.0, 1.0, None
    if isinstance(post_step, (tuple, list)) and len(post_step) == 2 and post_step[1] == "fix":
        return -_INF, _INF, _member(n, post_step[0], device)
    raise ValueError(f"post_step={post_step!r}: 'clamp01', 'clamp11', None or (fixed_rows, 'fix')")


def _propagate_tensor(g, y0, num_layers, alpha, adj, lo, hi, fixed, want_abs, ws=None):
    n = y0.shape[0]
    last = (1.0 - alpha) * y0
    y = y0
    clamp = lo != -_INF or hi != _INF
    if y0.is_cuda:
        from . import _C
        w = alpha * _edge_weights(g, adj, ws)
        d = g.csc
        step = lambda t: _C.spmm(d, t.unsqueeze(1), w, addend=last.unsqueeze(1)).view(n, -1)
    else:
        src, dst = g.edges()
        src_scale, dst_scale = _degree_scales(g, adj, ws)
        we = None if ws is None else ws["eid"][:, None]

        def step(t):
            if src_scale is not None:
                t = t * src_scale[:, None]
            h = torch.zeros_like(t).index_add_(0, dst, t[src] if we is None else t[src] * we)
            if dst_scale is not None:
                h = h * dst_scale[:, None]
            return alpha * h + last
    for _ in range(num_layers):
        y = step(y)
        if clamp:
            y = y.clamp(lo, hi)
        if fixed is not None:
            y = torch.where(fixed[:, None], y0, y)
    return y, (y.abs().sum(1) if want_abs else None)


def _propagate_kernel(g, y0, num_layers, alpha, adj, lo, hi, fixed, want_abs, ws=None):
    from . import _C
    n, C = y0.shape
    if num_layers == 0:
        return y0, (y0.abs().sum(1) if want_abs else None)
    start = y0.contiguous()
    d = g.csc
    src_scale, dst_scale = _degree_scales(g, adj, ws)
    kw = {} if ws is None else {"ew": ws["pos"]}       # without a weight the call is the one it was
    bufs = (torch.empty_like(start), torch.empty_like(start) if num_layers > 1 else None)
    fx = None if fixed is None else fixed.to(torch.uint8).contiguous()
    row_abs = torch.empty(n, dtype=torch.float32, device=y0.device) if want_abs else None
    partial = torch.empty(d.n_slots * C, dtype=torch.float32, device=y0.device) if d.n_long else None
    y = start
    for it in range(num_layers):
        out, last = bufs[it & 1], it == num_layers - 1
        # between sweeps the iterate stays multiplied by the source scale (out_scale): only the first sweep reads src_scale per edge
        _C.propagate_step(d, y, start, out, alpha, 1.0 - alpha, src_scale if it == 0 else None, dst_scale, lo, hi, fixed=fx,
                          row_abs=row_abs if last else None, out_scale=None if last else src_scale, partial=partial, **kw)
        y = out
    return y, row_abs


def propagate(g, y_start, num_layers, alpha, adj="DAD", post_step=None, impl=None, want_abs=False, edge_weight=None):
    """`num_layers` iterations of y <- post(alpha * P y + (1 - alpha) * y_start) from y = y_start (float32 [N, C] on g's device).
    Returns (y float32 [N, C], row_abs float32 [N] = sum_c |y[v, c]| or None).  No host read.
    `edge_weight`: float32 [E] / [E, 1] in edge-id order or an edata key (module docstring): finite and non-negative, not checked."""
    _square(g)
    if adj not in _ADJ:
        raise ValueError(f"adj={adj!r}: one of {_ADJ}")
    num_layers = int(num_layers)
    if num_layers < 0:
        raise ValueError("num_layers must be >= 0")
    n = g.number_of_nodes()
    if y_start.dim() != 2 or y_start.shape[0] != n:
        raise ValueError(f"the start matrix must be [{n}, C], got {tuple(y_start.shape)}")
    if y_start.device != g.device:
        raise ValueError(f"the start matrix lives on {y_start.device}, the graph on {g.device}")
    y_start = y_start.to(torch.float32)
    lo, hi, fixed = _post(post_step, n, y_start.device)
    ws = _weights(g, edge_weight)
    impl = default_impl(y_start, ws is not None) if impl is None else impl
    if impl not in ("kernel", "tensor"):
        raise ValueError(f"impl={impl!r}: 'kernel' or 'tensor'")
    run = _propagate_kernel if impl == "kernel" else _propagate_tensor
    C = y_start.shape[1]
    # on the GPU odd widths (41, 47 classes) would take 4-byte lanes and one row per wavefront; padded with zero columns (which stay zero
    # under every post step and add nothing to a row norm) they run with 16-byte lanes and several rows per wavefront (ops._pad4's rule)
    Cp = C if (not y_start.is_cuda or C % 4 == 0 or C < 5) else C + 4 - C % 4
    if Cp != C:
        y_start = torch.nn.functional.pad(y_start, (0, Cp - C))
    if ws is None:
        y, row_abs = run(g, y_start, num_layers, float(alpha), adj, lo, hi, fixed, want_abs)
    else:
        y, row_abs = run(g, y_start, num_layers, float(alpha), adj, lo, hi, fixed, want_abs, ws)
    return (y if Cp == C else y[:, :C].contiguous()), row_abs


class LabelPropagation:
    """`dgl.nn.LabelPropagation`: `lp(g, labels, mask=None, post_step="clamp01")` -> float32 [N, C].
    labels: int64 [N] / [N, 1] class ids (one-hot over labels.max() + 1 classes: one host read) or float [N, C]; with `mask` (index or bool
    [N]) the rows outside it start at zero.  post_step: "clamp01", "clamp11", None, or (fixed_rows, "fix") = those rows are reset to their
    start values after every iteration.  `edge_weight`: as `propagate`'s (finite, non-negative; not checked)."""

    def __init__(self, num_layers, alpha, adj="DAD", impl=None):
        if adj not in _ADJ:
            raise ValueError(f"adj={adj!r}: one of {_ADJ}")
        self.num_layers, self.alpha, self.adj, self.impl = int(num_layers), float(alpha), adj, impl

    @torch.no_grad()
    def __call__(self, g, labels, mask=None, post_step="clamp01", edge_weight=None):
        _square(g)
        labels = torch.as_tensor(labels)
        n = g.number_of_nodes()
        if labels.shape[0] != n:
            raise ValueError(f"labels must have one row per node ({n}), got {tuple(labels.shape)}")
        if labels.is_floating_point():
            if labels.dim() != 2:
                raise ValueError(f"float labels must be [N, C], got {tuple(labels.shape)}")
            y = labels.to(torch.float32)
        else:
            if labels.dim() > 2 or (labels.dim() == 2 and labels.shape[1] != 1):
                raise ValueError(f"integer labels must be [N] or [N, 1] (multi-class only), got {tuple(labels.shape)}")
            y = _onehot(labels, int(labels.max()) + 1 if n else 1, torch.float32, labels.device)
        if mask is not None:
            y = torch.where(_member(n, mask, y.device)[:, None], y, torch.zeros((), dtype=y.dtype, device=y.device))
        return propagate(g, y, self.num_layers, self.alpha, self.adj, post_step, self.impl, edge_weight=edge_weight)[0]


class CorrectAndSmooth:
    """Correct and Smooth.  `cs(g, y_soft, y_true, mask)` = `smooth(g, correct(g, y_soft, y_true, mask), y_true, mask)`:
    y_soft float [N, C] (the base predictor's class probabilities), y_true int [|mask|] / [|mask|, 1] (the class ids of the rows of
    `mask`, in mask order; ids outside [0, C) are not checked - that would be a host read), mask an index tensor or a bool [N].
    None of the defaults is tuned.  No host read in `correct` or `smooth`.  `edge_weight` (float32 [E] / [E, 1] in edge-id order or an
    edata key): both stages propagate with the weighted adjacency and the weighted in-degrees; the weights are expected finite and
    non-negative and, like the class ids, are not checked - that would be a host read."""

    def __init__(self, num_correction_layers=50, correction_alpha=0.8, correction_adj="DAD", num_smoothing_layers=50, smoothing_alpha=0.8,
                 smoothing_adj="DAD", autoscale=True, scale=1.0, impl=None):
        for adj in (correction_adj, smoothing_adj):
            if adj not in _ADJ:
                raise ValueError(f"adj={adj!r}: one of {_ADJ}")
        self.num_correction_layers, self.correction_alpha, self.correction_adj = int(num_correction_layers), float(correction_alpha), correction_adj
        self.num_smoothing_layers, self.smoothing_alpha, self.smoothing_adj = int(num_smoothing_layers), float(smoothing_alpha), smoothing_adj
        self.autoscale, self.scale, self.impl = bool(autoscale), float(scale), impl

    @staticmethod
    def _inputs(g, y_soft, y_true, mask):
        _square(g)
        n = g.number_of_nodes()
        if y_soft.dim() != 2 or y_soft.shape[0] != n or not y_soft.is_floating_point():
            raise ValueError(f"y_soft must be float [{n}, C], got {tuple(y_soft.shape)} {y_soft.dtype}")
        y_soft = y_soft.to(torch.float32)
        mask = torch.as_tensor(mask, device=y_soft.device)
        y_true = torch.as_tensor(y_true, device=y_soft.device)
        if y_true.dim() == 2 and y_true.shape[1] != 1:
            raise ValueError(f"y_true must be [n] or [n, 1] class ids (multi-class only), got {tuple(y_true.shape)}")
        if y_true.shape[0] == 0 or (mask.dtype != torch.bool and mask.numel() == 0):
            raise ValueError("Correct and Smooth needs at least one labelled row: the mask is empty")
        if mask.dtype != torch.bool and mask.numel() != y_true.shape[0]:
            raise ValueError(f"y_true has {y_true.shape[0]} rows for a mask of {mask.numel()}")
        onehot = _rows_to_full(n, mask, _onehot(y_true, y_soft.shape[1], torch.float32, y_soft.device))
        member = _member(n, mask, y_soft.device)
        count = member.sum() if mask.dtype == torch.bool else mask.numel()
        return y_soft, onehot, member, count

    @torch.no_grad()
    def correct(self, g, y_soft, y_true, mask, edge_weight=None):
        y_soft, onehot, member, count = self._inputs(g, y_soft, y_true, mask)
        E = torch.where(member[:, None], onehot - y_soft, torch.zeros((), dtype=torch.float32, device=y_soft.device))
        if self.autoscale:
            Eh, row_abs = propagate(g, E, self.num_correction_layers, self.correction_alpha, self.correction_adj, "clamp11", self.impl, want_abs=True,
                                     edge_weight=edge_weight)
            sigma = E.abs().sum() / count
            scale = sigma / row_abs
            scale = torch.where(torch.isinf(scale) | (scale > 1000.0), torch.ones((), dtype=scale.dtype, device=scale.device), scale)
            out = y_soft + scale[:, None] * Eh
        else:
            Eh, _ = propagate(g, E, self.num_correction_layers, self.correction_alpha, self.correction_adj, (member, "fix"), self.impl,
                              edge_weight=edge_weight)
            out = y_soft + self.scale * Eh
        return torch.where(torch.isfinite(out), out, y_soft)

    @torch.no_grad()
    def smooth(self, g, y_soft, y_true, mask, edge_weight=None):
        y_soft, onehot, member, _ = self._inputs(g, y_soft, y_true, mask)
        y = torch.where(member[:, None], onehot, y_soft)
        return propagate(g, y, self.num_smoothing_layers, self.smoothing_alpha, self.smoothing_adj, "clamp01", self.impl,
                         edge_weight=edge_weight)[0]

    def __call__(self, g, y_soft, y_true, mask, edge_weight=None):
        if edge_weight is None:
            return self.smooth(g, self.correct(g, y_soft, y_true, mask), y_true, mask)
        return self.smooth(g, self.correct(g, y_soft, y_true, mask, edge_weight), y_true, mask, edge_weight)


@torch.no_grad()
def evaluate_smoothed(model, graph, feat, labels, train_idx, val_idx, test_idx, cs, edge_weight=None, **evaluate_kw):
    """`train.evaluate`, then `cs` on the softmax of its predictions with the training labels:
    (train_acc, val_acc, test_acc, smoothed train_acc, val_acc, test_acc, smoothed [N, C] in original node order).  The six accuracies come
    from one `metrics.accuracy` call each over the split as groups and are read back once.  `edge_weight` is handed to `cs` (the model's
    evaluation takes none)."""
    from . import metrics, train
    pred = train.evaluate(model, graph, feat, labels, train_idx, val_idx, test_idx, **evaluate_kw)[-1]
    n = pred.shape[0]
    y_soft = torch.softmax(pred.float(), dim=-1)
    mask = train_idx
    if graph.node_perm is not None:            # the stacks speak original order, the propagation the graph's own numbering
        y_soft, mask = graph.to_internal(y_soft), graph.node_inv[train_idx]
    smoothed = cs(graph, y_soft, labels[train_idx], mask) if edge_weight is None else cs(graph, y_soft, labels[train_idx], mask, edge_weight)
    smoothed = graph.to_original(smoothed)
    groups = torch.full((n,), -1, dtype=torch.int8, device=pred.device)
    for code, idx in enumerate((train_idx, val_idx, test_idx)):
        groups.index_fill_(0, idx, code)
    lab = labels.view(n, 1)
    accs = torch.cat([metrics.accuracy(pred, lab, groups, 3), metrics.accuracy(smoothed, lab, groups, 3)]).tolist()   # the one host read
    return (*accs, smoothed)
