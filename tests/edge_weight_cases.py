"""Float64 / numpy restatements of the edge-weight contracts, shared by tests/test_edge_weight_host.py and
tests/test_edge_weight_gpu.py: `nn.GraphConv(edge_weight=)` and `nn.EdgeWeightNorm`, one `bot_propagate_step_w_f32` sweep and the full
weighted label-propagation / Correct and Smooth runs (tests/smooth_cases.py with the weight and the weighted degree rule),
`bot_subgraph_tally_i32` and `sampling.saint_norms`; and CPU stand-ins for `_C.subgraph_tally` and the weighted `_C.propagate_step`.
Nothing here calls the code under test."""
import functools

import numpy as np
import torch

from tests import saint_cases as SN
from tests import smooth_cases as SC

F64 = torch.float64
INF = SC.INF


# ------------------------------------------------------------------------------------------------ GraphConv / EdgeWeightNorm
def graphconv(src, dst, n_src, n_dst, feat, W, bias, ew, norm):
    """out = Din^p (A_w (Dout^-1/2 X)) W + b in float64, A_w[v, u] = the sum of ew over the edges u -> v; the degrees are STRUCTURAL
    (edge counts, clamped at 1), p = -1/2 ('both'), -1 ('right'), none ('none').  Differentiable in feat, W, bias and ew."""
    h = feat
    if norm == "both":
        dout = torch.bincount(src, minlength=n_src).to(F64).clamp(min=1)
        h = h * (dout ** -0.5)[:, None]
    msg = h[src] if ew is None else h[src] * ew.reshape(-1, 1)
    rst = torch.zeros((n_dst, h.shape[1]), dtype=F64).index_add(0, dst, msg)
    if W is not None:
        rst = rst @ W
    din = torch.bincount(dst, minlength=n_dst).to(F64).clamp(min=1)
    if norm == "both":
        rst = rst * (din ** -0.5)[:, None]
    elif norm == "right":
        rst = rst / din[:, None]
    return rst if bias is None else rst + bias


def edge_weight_norm(src, dst, n, w, norm, eps=0.0):
    w = w.to(F64).reshape(-1)
    if norm == "none":
        return w
    din = eps + torch.zeros(n, dtype=F64).index_add_(0, dst, w)
    if norm == "right":
        return w / din[dst]
    dout = eps + torch.zeros(n, dtype=F64).index_add_(0, src, w)
    return w / torch.sqrt(dout[src] * din[dst])


# ------------------------------------------------------------------------------------------------ weighted propagation
def scales(dst, n, adj, w):
    """smooth_cases.scales with the weighted in-degree: d[v] = s[v] if s[v] > 0 else 1, s[v] = the sum of w over the in-edges of v."""
    s = torch.zeros(n, dtype=F64).index_add_(0, dst, w.to(F64).reshape(-1))
    deg = torch.where(s > 0, s, torch.ones((), dtype=F64))
    return {"DAD": (deg ** -0.5, deg ** -0.5), "DA": (None, 1.0 / deg), "AD": (1.0 / deg, None), None: (None, None)}[adj]


def step(src, dst, w, y, y0, alpha, beta, src_scale, dst_scale, lo, hi, fixed=None):
    """smooth_cases.step with every term of the row's sum times w[e]: (out, row_abs, bound)."""
    y, y0, w = y.to(F64), y0.to(F64), w.to(F64).reshape(-1, 1)
    t = y if src_scale is None else y * src_scale.to(F64)[:, None]
    s = torch.zeros_like(y0).index_add_(0, dst, t[src] * w)
    mag = torch.zeros_like(y0).index_add_(0, dst, (t[src] * w).abs())
    if dst_scale is not None:
        s, mag = s * dst_scale.to(F64)[:, None], mag * dst_scale.to(F64)[:, None]
    out = (alpha * s + beta * y0).clamp(lo, hi)
    if fixed is not None:
        out = torch.where(fixed.bool()[:, None], y0, out)
    return out, out.abs().sum(1), abs(alpha) * mag + abs(beta) * y0.abs()


def propagate(src, dst, n, w, y_start, num_layers, alpha, adj, post_step):
    ss, ds = scales(dst, n, adj, w)
    if isinstance(post_step, tuple):
        lo, hi, fixed = -INF, INF, SC.member(n, post_step[0])
    else:
        (lo, hi), fixed = SC.POSTS[post_step], None
    y0 = y_start.to(F64)
    y = y0
    for _ in range(num_layers):
        y = step(src, dst, w, y, y0, alpha, 1.0 - alpha, ss, ds, lo, hi, fixed)[0]
    return y


def label_propagation(src, dst, n, w, labels, num_layers, alpha, adj="DAD", mask=None, post_step="clamp01"):
    y = labels.to(F64) if labels.is_floating_point() else SC.onehot(labels, int(labels.max()) + 1)
    if mask is not None:
        y = torch.where(SC.member(n, mask)[:, None], y, torch.zeros((), dtype=F64))
    return propagate(src, dst, n, w, y, num_layers, alpha, adj, post_step)


def correct_and_smooth(src, dst, n, w, y_soft, y_true, mask, num_layers=50, alpha=0.8, adj="DAD", autoscale=True, scale=1.0):
    """smooth_cases.correct_and_smooth on the weighted adjacency: (smoothed, raw autoscale factors or None)."""
    idx = SC._index(n, mask)
    y_soft = y_soft.to(F64)
    E = torch.zeros_like(y_soft)
    E[idx] = SC.onehot(y_true, y_soft.shape[1]) - y_soft[idx]
    if autoscale:
        Eh = propagate(src, dst, n, w, E, num_layers, alpha, adj, "clamp11")
        sigma = E[idx].abs().sum() / idx.numel()
        raw = sigma / Eh.abs().sum(1)
        s = torch.where(torch.isinf(raw) | (raw > 1000.0), torch.ones((), dtype=F64), raw)
        out = y_soft + s[:, None] * Eh
    else:
        raw = None
        out = y_soft + scale * propagate(src, dst, n, w, E, num_layers, alpha, adj, (idx, "fix"))
    c = torch.where(torch.isfinite(out), out, y_soft)
    y = c.clone()
    y[idx] = SC.onehot(y_true, y.shape[1])
    return propagate(src, dst, n, w, y, num_layers, alpha, adj, "clamp01"), raw


@functools.lru_cache(maxsize=None)
def weights(name, lo=0.5, hi=1.5, seed=0):
    """The fixture's edge weights, float32 [E] in the edge order of smooth_cases.graph(name): seeded uniform in [lo, hi)."""
    e = SC.graph(name)[0].numel()
    gen = torch.Generator().manual_seed(7919 * seed + e)
    return (lo + (hi - lo) * torch.rand(e, generator=gen)).to(torch.float32)


@functools.lru_cache(maxsize=None)
def cs_reference(name, C, adj, autoscale, alpha=0.8, num_layers=50):
    src, dst, n = SC.graph(name)
    y_soft, y_true, mask = SC.cs_inputs(name, C)
    return correct_and_smooth(src, dst, n, weights(name), y_soft, y_true, mask, num_layers, alpha, adj, autoscale)


@functools.lru_cache(maxsize=None)
def lp_reference(name, C, adj, alpha=0.8, num_layers=50):
    src, dst, n = SC.graph(name)
    _, y_true, mask = SC.cs_inputs(name, C)
    labels = torch.zeros(n, dtype=torch.int64)
    labels[mask] = y_true
    labels[0] = C - 1
    return labels, label_propagation(src, dst, n, weights(name), labels, num_layers, alpha, adj, mask=mask)


# ------------------------------------------------------------------------------------------------ tally / saint_norms
def tally_reference(indptr, indices, node_sets, tally=None):
    """int32 [nnz]: for every set and every listed node, +1 at the CSC positions of its row whose source is in the set too."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    tally = np.zeros(len(indices), dtype=np.int32) if tally is None else tally
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr))
    for nodes in node_sets:
        member = np.zeros(len(indptr) - 1, dtype=bool)
        member[np.asarray(nodes, dtype=np.int64)] = True
        tally += (member[rows] & member[indices]).astype(np.int32)
    return tally


def saint_norms_reference(g, sampler, n_presample, seed=0):
    """(loss_weight float32 [N] original order, edge_norm float32 [E] edge-id order, sets as g's OWN ids, C int64 [N] own ids,
    T int64 [E] edge-id order)."""
    c = g.csc
    indptr, indices, eid = (a.cpu().numpy().astype(np.int64) for a in (c.indptr, c.indices, c.eid))
    n = g.number_of_nodes()
    sets = [SN.sampler_nodes_reference(g, sampler, s).astype(np.int64) for s in SN.presample_seeds(n_presample, seed)]
    count = np.zeros(n, dtype=np.int64)
    for s in sets:
        count[s] += 1
    T = tally_reference(indptr, indices, sets).astype(np.int64)
    rows = np.repeat(np.arange(n), np.diff(indptr))
    pos = np.where(T > 0, count[rows].astype(np.float32) / np.maximum(T, 1).astype(np.float32), np.float32(1.0)).astype(np.float32)
    edge_norm = np.empty_like(pos)
    edge_norm[eid] = pos
    T_eid = np.empty_like(T)
    T_eid[eid] = T
    lw = (np.float32(n_presample) / np.maximum(count, 1).astype(np.float32)).astype(np.float32)
    if g.node_perm is not None:
        out = np.empty_like(lw)
        out[g.node_perm.cpu().numpy()] = lw
        lw = out
    return lw, edge_norm, sets, count, T_eid


# ------------------------------------------------------------------------------------------------ CPU stand-ins for the _C wrappers
def subgraph_tally_standin(csc, nodes, node_map, tally):
    assert tally.dtype == torch.int32 and tally.numel() == csc.nnz and bool((node_map == -1).all())
    got = tally_reference(csc.indptr.cpu().numpy(), csc.indices.cpu().numpy(), [nodes.cpu().numpy()])
    tally += torch.from_numpy(got).to(tally.device)
    return tally


def propagate_step_standin(d, y, y0, out, alpha, beta, src_scale, dst_scale, lo, hi, fixed=None, row_abs=None, out_scale=None, partial=None,
                           ew=None):
    """_C.propagate_step on CPU tensors in float32 tensor ops (ew: CSC position order), with the kernel's order of the per-edge product:
    fl(ew * src_scale) first."""
    n, C = y.shape
    rows = torch.repeat_interleave(torch.arange(n), (d.indptr[1:] - d.indptr[:-1]).long())
    idx = d.indices.long()
    sv = torch.ones(idx.numel()) if src_scale is None else src_scale[idx]
    if ew is not None:
        sv = sv * ew
    s = torch.zeros((n, C)).index_add_(0, rows, sv[:, None] * y[idx])
    av = alpha * (dst_scale if dst_scale is not None else torch.ones(n))
    o = (av[:, None] * s + beta * y0).clamp(lo, hi)
    if fixed is not None:
        o = torch.where(fixed.bool()[:, None], y0, o)
    if row_abs is not None:
        row_abs.copy_(o.abs().sum(1))
    out.copy_(o if out_scale is None else o * out_scale[:, None])
    return out
