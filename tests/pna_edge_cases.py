"""Float64 restatements of the PNA contracts with edge features (include/bot_gnn.h "PNA aggregation with edge features"),
shared by tests/test_pna_edge_host.py and tests/test_pna_edge_gpu.py: the per-position messages m_k = a[u_k] + W_e ef_k (+ b[v]), the
aggregators over them, the owner positions of max and min, what the rounding bounds of the kernel's summation order need, the autograd
of the same formula evaluated at given owners, and `EdgePNAConv` / `EdgePNA` written the way DGL writes them: M(cat[h_u, h_v, e]) per
edge.  The restatements call nothing of the code under test; the `check_*` functions at the end run a layer or a stack against them
on whatever device the graph lives on.  Scalers, layout, BatchNorm and the graphs are tests/pna_cases.py's and tests/sage_cases.py's."""
import math

import numpy as np
import torch

from tests import pna_cases as PC
from tests import sage_cases as SG

F64 = torch.float64
U32 = PC.U32


def position_rows(g):
    """int64 [E]: the row of an edge-id-ordered edge tensor for every CSC position (a batch graph's edge ids ARE its positions)."""
    eid = getattr(g.csc, "eid", None)
    from bot_amd.sampling import _BatchGraph
    if isinstance(g, _BatchGraph) or eid is None:
        return np.arange(g.number_of_edges(), dtype=np.int64)
    return eid.cpu().numpy().astype(np.int64)


def csr_of(g):
    """(indptr, indices, position in the CSC of every CSR position) as numpy arrays."""
    return g.csr.indptr.cpu().numpy(), g.csr.indices.cpu().numpy(), g.csr2csc.cpu().numpy()


# ------------------------------------------------------------------------------------------------ the aggregation, numpy float64
def edge_terms(ef_pos, weight):
    """(c, C) float64 [E, F]: c_k = sum_j ef_kj w_fj and C_k = sum_j |ef_kj w_fj| from the float32 operands."""
    e64, w64 = ef_pos.astype(np.float64), weight.astype(np.float64)
    return e64 @ w64.T, np.abs(e64) @ np.abs(w64).T


def first_owner(seg_vals, lo, sign):
    """The smallest position of a row's [deg, F] values that attains the max (sign 1) or the min (sign -1); -0.0 == +0.0."""
    v = sign * seg_vals
    return lo + np.argmax(v == v.max(0), axis=0)


def aggregate(indptr, indices, a, ef_pos, weight, b):
    """Every aggregator of m_k = a[u_k] + c_k + b[v] per row in float64 on the messages themselves (two passes for the variance), the
    owner positions of max and min (of a_k + c_k: b is a row constant), and what the bounds need.  Returns (vals {name: [n, F]},
    (argmax, argmin) int32 [n, F], info) with info: deg [n]; D = max_k (|a_k - a_0| + |c_k - c_0|); a0, c0, babs; asum = sum_k (|a_k| +
    |c_k|); Cmax = max_k C_k, Csum = sum_k C_k, C0; aC = max_k (|a_k| + C_k); Dm = max_k |m_k - m_0|.  Empty rows are 0, positions
    -1."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    n, F = len(indptr) - 1, a.shape[1]
    a64 = a.astype(np.float64)
    b64 = np.zeros((n, F)) if b is None else b.astype(np.float64)
    c, C = edge_terms(ef_pos, weight)
    vals = {k: np.zeros((n, F)) for k in ("mean", "sum", "max", "min", "std", "var")}
    info = {k: np.zeros((n, F)) for k in ("D", "a0", "c0", "asum", "Cmax", "Csum", "C0", "aC", "Dm")}
    info["deg"], info["babs"] = np.diff(indptr), np.abs(b64)
    amax, amin = np.full((n, F), -1, dtype=np.int32), np.full((n, F), -1, dtype=np.int32)
    for r in range(n):
        lo, hi = indptr[r], indptr[r + 1]
        if hi == lo:
            continue
        rows, cr, Cr = a64[indices[lo:hi]], c[lo:hi], C[lo:hi]
        ac = rows + cr
        m = ac + b64[r]
        mean = m.mean(0)
        var = np.maximum(((m - mean) ** 2).mean(0), 0.0)
        vals["mean"][r], vals["sum"][r], vals["max"][r], vals["min"][r] = mean, m.sum(0), m.max(0), m.min(0)
        vals["var"][r], vals["std"][r] = var, np.sqrt(var + 1e-30)
        amax[r], amin[r] = first_owner(ac, lo, 1.0), first_owner(ac, lo, -1.0)
        info["D"][r] = (np.abs(rows - rows[0]) + np.abs(cr - cr[0])).max(0)
        info["Dm"][r] = np.abs(ac - ac[0]).max(0)
        info["a0"][r], info["c0"][r], info["C0"][r] = np.abs(rows[0]), np.abs(cr[0]), Cr[0]
        info["asum"][r] = (np.abs(rows) + np.abs(cr)).sum(0)
        info["Cmax"][r], info["Csum"][r], info["aC"][r] = Cr.max(0), Cr.sum(0), (np.abs(rows) + Cr).max(0)
    return vals, (amax, amin), info


def bounds(info, K):
    """The rounding bounds of the kernel's order (u = 2^-24; the issue's, which follow from the contract's order: the chain of K
    roundings per edge term, the split-pivot deviations, position-order sums, P + S1 / n and S1 + n P + n b):
        mean  (deg + 4) u (D + |a_0| + |c_0| + |b|) + 2 K u max C
        sum   (deg + 4) u (sum_k (|a_k| + |c_k|) + deg (|a_0| + |c_0| + |b|)) + 2 K u (sum_k C_k + deg C_0)
        var   (3 deg + 16) u D^2 + 8 K u D max C
        ext   (K + 3) u (max_k (|a_k| + C_k) + |b|)                                                        for max and for min"""
    deg = info["deg"][:, None].astype(np.float64)
    base = info["a0"] + info["c0"] + info["babs"]
    return {"mean": (deg + 4) * U32 * (info["D"] + base) + 2 * K * U32 * info["Cmax"],
            "sum": (deg + 4) * U32 * (info["asum"] + deg * base) + 2 * K * U32 * (info["Csum"] + deg * info["C0"]),
            "var": (3 * deg + 16) * U32 * info["D"] ** 2 + 8 * K * U32 * info["D"] * info["Cmax"],
            "ext": (K + 3) * U32 * (info["aC"] + info["babs"])}


def forward(indptr, indices, a, ef_pos, weight, b, aggregators, scalers, delta, Ft=None):
    """out float64 [n, S*A*F] of the contract, with (argmax, argmin)."""
    vals, own, _ = aggregate(indptr, indices, a, ef_pos, weight, b)
    stack = np.stack([vals[k] for k in aggregators])
    return PC.layout(stack, PC.scale_table(indptr, scalers, delta), Ft or a.shape[1]), own


# ------------------------------------------------------------------------------------------------ the same formula, float64 autograd
def aggregate_messages(indptr, msg, aggregators, scalers, delta, Ft=None, argmax=None, argmin=None):
    """The aggregators, scalers and tower layout over per-POSITION float64 messages msg [E, F] (destination term included) as
    differentiable torch ops: var is the mean of the squared deviations through relu (gradient 0 at 0: the var == 0 gate); with
    `argmax` / `argmin` ([n, F] CSC positions, -1 = none) max and min are evaluated AT those owners."""
    indptr_t = torch.as_tensor(np.asarray(indptr, dtype=np.int64))
    n, F = indptr_t.numel() - 1, msg.shape[1]
    deg = indptr_t[1:] - indptr_t[:-1]
    seg = torch.repeat_interleave(torch.arange(n), deg)
    some = (deg > 0).reshape(-1, 1)
    cnt = deg.clamp(min=1).to(F64).reshape(-1, 1)
    zero = torch.zeros((), dtype=F64)
    total = torch.zeros((n, F), dtype=F64).index_add(0, seg, msg)
    mean = total / cnt
    var = torch.relu(torch.zeros((n, F), dtype=F64).index_add(0, seg, (msg - mean[seg]) ** 2) / cnt)

    def extreme(arg, sign):
        if arg is None:
            idxs = seg.reshape(-1, 1).expand(-1, F)
            return sign * torch.zeros((n, F), dtype=F64).scatter_reduce(0, idxs, sign * msg, "amax", include_self=False)
        pos = torch.as_tensor(np.asarray(arg)).long()
        return torch.where(pos >= 0, msg.gather(0, pos.clamp(min=0)), zero)
    val = {"mean": mean, "sum": total, "var": var, "std": torch.sqrt(var + 1e-30)}
    if "max" in aggregators:
        val["max"] = extreme(argmax, 1.0)
    if "min" in aggregators:
        val["min"] = extreme(argmin, -1.0)
    vals = torch.stack([torch.where(some, val[k], zero) for k in aggregators], dim=1)          # [n, A, F]
    scale = torch.from_numpy(PC.scale_table(indptr, scalers, delta))                           # [S, n]
    S, A, Ft = scale.shape[0], len(aggregators), Ft or F
    v = vals.reshape(n, 1, A, F // Ft, Ft) * scale.t().reshape(n, S, 1, 1, 1)
    return v.permute(0, 3, 1, 2, 4).reshape(n, S * A * F)


def pna_edge_torch(indptr, indices, a, b, ef_pos, weight, aggregators, scalers, delta, Ft=None, argmax=None, argmin=None):
    """The contract as float64 autograd: a [n_src, F], b [n, F] or None, ef_pos [E, K] (position order), weight [F, K]."""
    indptr_t = torch.as_tensor(np.asarray(indptr, dtype=np.int64))
    idx = torch.as_tensor(np.asarray(indices, dtype=np.int64))
    seg = torch.repeat_interleave(torch.arange(indptr_t.numel() - 1), indptr_t[1:] - indptr_t[:-1])
    msg = a[idx] + ef_pos @ weight.t()
    if b is not None:
        msg = msg + b[seg]
    return aggregate_messages(indptr, msg, aggregators, scalers, delta, Ft, argmax, argmin)


def exact_backward(indptr, indices, a, ef_pos, weight, aggregators, dout, amax, amin):
    """(da, db, dweight) float64 of integer operands for sum / max / min with one scaler of ones and one tower, written as loops over
    the edges; asserts that every partial sum of magnitudes stays below 2^24, so that float32 sums are exact in ANY order."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    n, F, K = len(indptr) - 1, a.shape[1], ef_pos.shape[1]
    d = dout.astype(np.float64).reshape(n, len(aggregators), F)
    deg = np.diff(indptr)
    seg = np.repeat(np.arange(n), deg)
    pos = np.arange(len(indices))[:, None]
    dm = np.zeros((len(indices), F))
    db = np.zeros((n, F))
    for i, k in enumerate(aggregators):
        if k == "sum":
            dm += d[seg, i]
            db += deg[:, None] * d[:, i]
        elif k in ("max", "min"):
            own = amax if k == "max" else amin
            dm += np.where(own[seg] == pos, d[seg, i], 0.0)
            db += np.where(deg[:, None] > 0, d[:, i], 0.0)
        else:
            raise ValueError(k)
    order = np.argsort(indices, kind="stable")                         # the edges of every source, one after the other
    starts = np.searchsorted(indices[order], np.arange(a.shape[0]))
    has = np.diff(np.append(starts, len(indices))) > 0

    def per_source(x):
        out = np.zeros((a.shape[0], F))
        if len(indices):
            out[has] = np.add.reduceat(x[order], starts[has], axis=0)
        return out
    da, da_abs = per_source(dm), per_source(np.abs(dm))
    e64 = ef_pos.astype(np.float64)
    dweight = dm.T @ e64
    assert max(float(da_abs.max()), float((np.abs(dm).T @ np.abs(e64)).max()), float(np.abs(db).max())) < 2.0 ** 24
    return da, db, dweight


def std_gradient_terms(indptr, indices, a, ef_pos, weight, aggregators, scalers, delta, Ft, dout):
    """What float32 under the contract's order may add to the std / var part of a gradient, per entry, from the float64 restatement
    alone -> (term_da [n_src, F], term_dweight [F, K]).  Per edge e = (u -> v) and column the std / var part of dm is c1 dev with
    dev = m_e - mean_v and c1 = G_std / (n std) + 2 G_var / n (G the dout of the aggregator folded over the scalers; 0 where var = 0).
      dev    formed as fl(fl(a - mu) + c): the rounding of mu, of the difference, of the sum and the chain's K roundings of c -
             |delta dev| <= (K + 4) u (|a_u| + C_e + |mean_v|)
      std    every deviation of the forward, d_k = fl(fl(a_k - a_0) + fl(c_k - c_0)), carries at most eps = 3 u D + 2 K u max C; the
             standard deviation moves by at most the largest change of a value, so by eps; S2 / n - (S1 / n)^2 in float32 adds at most
             2 (deg + 4) u Dm^2 to var (Dm = max_k |m_k - m_0|), i.e. (deg + 4) u Dm^2 / std to std, and the root 2 u std:
             delta std <= eps + (deg + 4) u Dm^2 / std + 2 u std,  rho = delta std / std,
             |delta c1| <= |G_std| / (n std) rho / (1 - rho)   (no bound from rho = 1 on: the entry's term is infinite)
    tau_e = |c1| |delta dev| + |dev| |delta c1|;  term_da[u] = the sum of tau_e over the out-edges of u, term_dweight[f, j] = the sum
    over all edges of |ef_ej| tau_e[f].  On a row of ordinary spread the terms are a few u of the gradient; they grow only where a
    row's messages lie together (std far below D), where the gradient of std is ill-conditioned in its float32 inputs."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    n, F, K = len(indptr) - 1, a.shape[1], ef_pos.shape[1]
    vals, _, info = aggregate(indptr, indices, a, ef_pos, weight, None)
    c, C = edge_terms(ef_pos, weight)
    deg = info["deg"][:, None].astype(np.float64)
    cnt = np.maximum(deg, 1.0)
    seg = np.repeat(np.arange(n), info["deg"])
    scale = PC.scale_table(indptr, scalers, delta)                                             # [S, n]
    S, A, T = scale.shape[0], len(aggregators), F // Ft
    d = np.asarray(dout, dtype=np.float64).reshape(n, T, S, A, Ft)

    def folded(name):
        if name not in aggregators:
            return np.zeros((n, F))
        return (d[:, :, :, aggregators.index(name), :] * scale.T[:, None, :, None]).sum(2).reshape(n, F)
    live = vals["var"] > 0
    std = np.where(live, vals["std"], 1.0)
    c1_std = np.where(live, np.abs(folded("std")) / (cnt * std), 0.0)
    c1_var = np.where(live, 2.0 * np.abs(folded("var")) / cnt, 0.0)
    eps = 3 * U32 * info["D"] + 2 * K * U32 * info["Cmax"]
    rho = (eps + (deg + 4) * U32 * info["Dm"] ** 2 / std + 2 * U32 * std) / std
    with np.errstate(divide="ignore", invalid="ignore"):
        d_c1 = np.where(live & (c1_std > 0), np.where(rho < 1, c1_std * rho / np.maximum(1 - rho, 1e-300), np.inf), 0.0)
    a64 = a.astype(np.float64)[indices]
    dev = np.abs(a64 + c - vals["mean"][seg])
    d_dev = (K + 4) * U32 * (np.abs(a64) + C + np.abs(vals["mean"][seg]))
    tau = (c1_std + c1_var)[seg] * d_dev + np.where(d_c1[seg] > 0, dev * d_c1[seg], 0.0)
    term_da = np.zeros((a.shape[0], F))
    np.add.at(term_da, indices, tau)
    finite = np.where(np.isfinite(tau), tau, 0.0)
    term_dw = finite.T @ np.abs(ef_pos.astype(np.float64))
    hit = ~np.isfinite(tau)
    if hit.any():                                                      # an unbounded edge makes the weights of its column unbounded
        cols = np.nonzero(hit.any(0))[0]
        term_dw[cols] = np.where(np.abs(ef_pos[hit[:, cols].any(1)]).sum(0) > 0, np.inf, term_dw[cols])
    return term_da, term_dw


# ------------------------------------------------------------------------------------------------ EdgePNAConv and EdgePNA, float64
def edge_pna_conv(conv, indptr, indices, h_src, h_dst, ef_pos, p, sarg=None, training=False):
    """`EdgePNAConv` in float64 the way DGL writes it: per tower the message M(cat[h_u, h_v, e_uv]) on every edge (every tower sees the
    whole edge feature), the aggregation, U(cat[h, h_neigh]) / sqrt(n_dst), BatchNorm; the towers side by side, the mixing layer, the
    residual.  p: the layer's parameters as float64 tensors; sarg: the layer's [n_dst, 2 F] owner positions, or None."""
    T, Ft = conv.num_towers, conv.tower_in_size
    n_dst, F = h_dst.shape[0], conv.in_size
    indptr_t = torch.as_tensor(np.asarray(indptr, dtype=np.int64))
    idx = torch.as_tensor(np.asarray(indices, dtype=np.int64))
    seg = torch.repeat_interleave(torch.arange(n_dst), indptr_t[1:] - indptr_t[:-1])
    outs = []
    for t in range(T):
        hs, hd = h_src[:, t * Ft:(t + 1) * Ft], h_dst[:, t * Ft:(t + 1) * Ft]
        msg = PC._lin(torch.cat([hs[idx], hd[seg], ef_pos], dim=1), p, f"towers.{t}.M")           # M(cat[h_u, h_v, e]) per edge
        amax = None if sarg is None else sarg[:, t * Ft:(t + 1) * Ft]
        amin = None if sarg is None else sarg[:, F + t * Ft:F + (t + 1) * Ft]
        h_neigh = aggregate_messages(indptr, msg, conv.aggregators, conv.scalers, conv.delta, None, amax, amin)
        z = PC._lin(torch.cat([hd, h_neigh], dim=1), p, f"towers.{t}.U") / math.sqrt(n_dst)
        outs.append(PC._bn(z, p, f"towers.{t}.batchnorm", conv.towers[t].batchnorm, training))
    h = torch.nn.functional.leaky_relu(PC._lin(torch.cat(outs, dim=1), p, "mixing_layer.0"), 0.01)
    return h + h_dst if conv.residual else h


def edge_pna_stack(model, layers, feat, p, sargs=None):
    """`EdgePNA` (eval mode) in float64.  layers: per layer (indptr, indices, n_dst, ef_pos float64)."""
    h = PC._lin(feat, p, "encoder")
    for i, (indptr, indices, n_dst, ef_pos) in enumerate(layers):
        pre = f"convs.{i}."
        pi = {k[len(pre):]: v for k, v in p.items() if k.startswith(pre)}
        h = edge_pna_conv(model.convs[i], indptr, indices, h, h[:n_dst], ef_pos, pi, None if sargs is None else sargs[i])
        if i < len(layers) - 1:
            h = torch.relu(h)
    return PC._lin(h, p, "decoder")


# ------------------------------------------------------------------------------------------------ checks shared by both suites
class Spy:
    """Records the owner positions of every `ops.pna_aggregate_edge` call of the layers while active, and counts the edge-less calls."""

    def __init__(self, monkeypatch):
        from bot_amd import ops
        self.sarg, self.calls, self.plain = [], 0, 0
        real = getattr(ops.pna_aggregate_edge, "real", ops.pna_aggregate_edge)
        plain = getattr(ops.pna_aggregate, "real", ops.pna_aggregate)

        def pna_aggregate_edge(g, a, b, ef, weight, *args, **kw):
            kw["return_saved"] = True
            out, saved, sarg = real(g, a, b, ef, weight, *args, **kw)
            self.calls += 1
            self.sarg.append(sarg.cpu().numpy())
            return out

        def pna_aggregate(*args, **kw):
            self.plain += 1
            return plain(*args, **kw)
        pna_aggregate_edge.real, pna_aggregate.real = real, plain
        monkeypatch.setattr(ops, "pna_aggregate_edge", pna_aggregate_edge)
        monkeypatch.setattr(ops, "pna_aggregate", pna_aggregate)


def conv_keys(in_size, out_size, towers, K, n_blocks):
    """The state_dict of `EdgePNAConv`: DGL's names and shapes, M over [h_u | h_v | e]."""
    Ft, Fo = in_size // towers, out_size // towers
    want = {"mixing_layer.0.weight": (out_size, out_size), "mixing_layer.0.bias": (out_size,)}
    for t in range(towers):
        want.update({f"towers.{t}.M.weight": (Ft, 2 * Ft + K), f"towers.{t}.M.bias": (Ft,), f"towers.{t}.U.weight": (Fo, (n_blocks + 1) * Ft),
                     f"towers.{t}.U.bias": (Fo,), f"towers.{t}.batchnorm.weight": (Fo,), f"towers.{t}.batchnorm.bias": (Fo,),
                     f"towers.{t}.batchnorm.running_mean": (Fo,), f"towers.{t}.batchnorm.running_var": (Fo,),
                     f"towers.{t}.batchnorm.num_batches_tracked": ()})
    return want


def check_conv(g, dev, monkeypatch, in_size, out_size, towers, K, residual=True, aggregators=PC.AGGS4, scalers=PC.SCALERS3, seed=0, impl=None):
    """One `EdgePNAConv` forward + backward in eval mode on `g` against `edge_pna_conv` evaluated at the layer's own owner positions,
    under the suite's criteria (tests/parity_cases.py): the output, the input gradient and every parameter's gradient; exactly ONE
    aggregation call per forward; the state_dict key set and shapes."""
    from bot_amd import nn as bnn
    from tests.parity_cases import fwd_close, grad_close
    indptr, indices = SG.csc_of(g)
    n_src, n_dst, E = g.number_of_src_nodes(), g.number_of_dst_nodes(), g.number_of_edges()
    torch.manual_seed(seed)
    conv = bnn.EdgePNAConv(in_size, out_size, aggregators, scalers, delta=1.7, num_towers=towers, edge_feat_size=K, residual=residual)
    assert {k: tuple(v.shape) for k, v in conv.state_dict().items()} == conv_keys(in_size, out_size, towers, K, len(aggregators) * len(scalers))
    PC.randomise(conv, seed + 1)
    conv = conv.to(dev).eval()
    gen = torch.Generator().manual_seed(seed + 2)
    feat = torch.randn(n_src, in_size, generator=gen).to(dev).requires_grad_()
    ef = torch.randn(E, K, generator=gen)
    dout = torch.randn(n_dst, out_size, generator=gen)
    spy = Spy(monkeypatch)
    out = conv(g, feat, ef.to(dev)) if impl is None else conv(g, feat, ef.to(dev), impl=impl)
    assert spy.calls == 1 and spy.plain == 0 and out.shape == (n_dst, out_size)
    out.backward(dout.to(dev))
    p = SG.params64(conv)
    f64 = feat.detach().cpu().double().requires_grad_()
    sarg = spy.sarg[0]
    SG.check_arg(indptr, sarg)
    ef_pos = ef.double()[torch.from_numpy(position_rows(g))]
    ref = edge_pna_conv(conv, indptr, indices, f64, f64[:n_dst], ef_pos, p, sarg)
    ref.backward(dout.double())
    fwd_close(out, ref.detach().numpy())
    grad_close(feat.grad, f64.grad.numpy())
    for name, prm in conv.named_parameters():
        grad_close(prm.grad, p[name].grad.numpy())
    return conv


def check_stack(model, graphs, feat, edge_feats, dev, monkeypatch):
    """`EdgePNA` in eval mode on a Graph (edge_feats: a tensor) or a block list (a list of one tensor per block) against
    `edge_pna_stack` at the layers' own owner positions: output, input gradient and every parameter's gradient."""
    from tests.parity_cases import fwd_close, grad_close
    blocks = graphs if isinstance(graphs, (list, tuple)) else None
    per_layer = list(blocks) if blocks is not None else [graphs] * model.n_layers
    efs = list(edge_feats) if blocks is not None else [edge_feats] * model.n_layers
    PC.randomise(model, 5)
    model = model.to(dev).eval()
    model.zero_grad(set_to_none=True)
    x = feat.detach().clone().to(dev).requires_grad_()
    spy = Spy(monkeypatch)
    out = model(graphs, x, [e.to(dev) for e in efs] if blocks is not None else edge_feats.to(dev))
    assert spy.calls == model.n_layers and spy.plain == 0
    dout = torch.randn(out.shape, generator=torch.Generator().manual_seed(12))
    out.backward(dout.to(dev))
    p = SG.params64(model)
    f64 = feat.detach().cpu().double().requires_grad_()
    layers = [SG.csc_of(g) + (g.number_of_dst_nodes(), e.detach().cpu().double()[torch.from_numpy(position_rows(g))])
              for g, e in zip(per_layer, efs)]
    ref = edge_pna_stack(model, layers, f64, p, spy.sarg)
    ref.backward(dout.double())
    fwd_close(out, ref.detach().numpy())
    grad_close(x.grad, f64.grad.numpy())
    for name, prm in model.named_parameters():
        grad_close(prm.grad, p[name].grad.numpy())
