"""Differentiable sparse operators over a `bot_amd.Graph`, each backed by hand-written gfx950 kernels
through the C ABI (include/bot_gnn.h).  They replace the `dgl.ops` calls the reference makes
(SURVEY §2.1): copy_u_sum, u_mul_e_sum, copy_e_sum, copy_u, u_add_v, edge_softmax (+ `eids`), and add
the fused attention op the layers use (`gat_attention`: logits + leaky-ReLU + softmax in one sweep).

Edge tensors cross this API in edge-id order, like DGL's.  `gat_attention` / `u_mul_e_sum` also accept
`order="csc"`: the attention weights then stay in destination-major position order between the two
ops (no permutation gathers); the layers in `bot_amd.nn` use that form.

Backward formulas (hand-derived; checked against autograd of the oracle's forward definitions):
  copy_u_sum      dx = copy_u_sum on the reversed graph (CSR sweep)
  copy_u_max      dx[u] = sum_{e: u->v} dout[v] * (arg[v] == position of e)  (CSR sweep; no atomics)
  pna_aggregate   G_g[v] = sum_s scale_s[v] dout[v, block (s, g)];  db[v] = sum of G_g over mean, max, min (+ n G_g for sum);
                  da[u] = sum_{e: u->v} G_mean/n + G_sum + c1[v] (a[u] - mean[v]) + G_max (argmax[v] == position of e) + G_min (argmin[v] == ...),
                  c1 = G_std / (n std) + 2 G_var / n, 0 where var == 0  (a dense pass, then one CSR sweep; no atomics)
  copy_u_softmax  dx[u] = gate_u sum_{e: u->v} dout[v] * exp(beta m_u - lse[v]) * (1 + beta (m_u - out[v]))  (CSR sweep; no atomics);
                  dbeta = sum_{v,f} dout * (q - out^2)  (the weighted variance of the messages; a dense reduction)
  u_add_e_softmax dz_e = gate_e dout[v] * exp(beta m_e - lse[v]) * (1 + beta (m_e - out[v])) per edge e = u -> v, z and m formed again in the sweep;
                  dx[u] = sum_{e: u->v} dz_e,  dweight[f,j] = sum_e ef[e,j] dz_e[f]  (one persistent CSR sweep; no atomics);
                  dbias = sum_u dx[u],  dbeta as copy_u_softmax  (dense reductions)
  u_mul_e_sum     dx[u] = sum_{e: u->v} a_e * dout[v]  (CSR sweep, weights through csr2csc);
                  da_e  = <x[u], dout[v]>              (SDDMM dot, CSC sweep)
  gatv2_logits    t = de * attn * lrelu'(fs[u] + fd[v]);  dfd[v] = sum_in t (CSC sweep);  dfs[u] = sum_out t (CSR sweep, de through
                  csr2csc);  dattn = sum_e de * lrelu(fs[u] + fd[v]) (a by-product of the CSC sweep; no atomics)
  gated_sum       g = sigmoid(k[v] + q[u]), g' = g (1 - g);  a = dout (normalised: dout / (den + eps)), b = 0 (normalised: -a out);
                  ds_e = g' (v[u] a[v] + b[v]);  dk[v] = sum_in ds (CSC sweep);  dq[u] = sum_out ds,  dv[u] = sum_out g a[v]  (one CSR
                  sweep; the gates are formed again, nothing saved per edge, no atomics)
  gated_edge_sum  e = k[v] + q[u] + c_e (stored: the second output), g, g' from the stored e, a and b as gated_sum;
                  ds_e = de_e + g' (v[u] a[v] + b[v]) = dc_e;  dk[v] = sum_in ds (one CSC sweep);  dq[u] = sum_out ds,  dv[u] = sum_out g a[v]
                  (one CSR sweep, ds and e through csr2csc; no atomics)
  rel_expand_sum  dx[u] = sum_{e: u->v} c_e sum_b coef[r_e, b] dZ[v, b]  (`rel_contract_sum`'s sweep over the CSR);  dcoef[r, b] = sum_{e: r_e = r}
                  c_e <x[u], dZ[v, b]>  (SDDMM dots [E, B], then a segment sum over the relations as rows; no atomics).  `rel_contract_sum`
                  is the transpose: dy[u, b] = sum_e c_e coef[r_e, b] dout[v]  (the expand sweep over the CSR), dcoef with <y[u, b], dout[v]>
  dot_attention   delta_v = <dout[v], out[v]>;  ds_k = a_k (c keep_k <dout[v], v[u_k]> - delta_v);  dq[v] = scale sum_in ds k[u] (CSC sweep);
                  dk[u] = scale sum_out ds q[v],  dv[u] = sum_out c keep a dout[v]  (one CSR sweep, p and ds through csr2csc; no atomics)
  appnp_propagate g_k = dout;  g_{t-1} = (1 - alpha) P_t^T g_t;  dx = g_0;  dh0 = alpha sum_t g_t  (bot_amd/appnp.py: k CSR sweeps, the masks
                  regenerated from the seed, the sum in the sweeps' epilogue; nothing saved, no atomics)
  gat_attention   t_v = sum a*da;  de = a*(da - t_v);  dz = de * leaky'(z);
                  d_er[v] = sum_in dz;  d_el[u] = sum_out dz;  d_ee = dz
"""
from __future__ import annotations

import os
import weakref
from collections import namedtuple

import torch

from . import _C
from .graph import _TAKE_CHUNK, take_rows

__all__ = ["copy_u_sum", "u_mul_e_sum", "copy_e_sum", "copy_u", "u_add_v", "edge_softmax", "gat_attention", "copy_u_max", "gatv2_logits", "copy_u_softmax", "u_add_e_softmax", "dot_attention_edge",
           "dot_attention", "pna_aggregate", "pna_aggregate_edge", "copy_u_min", "appnp_propagate", "appnp_keep", "gated_sum", "gated_edge_sum", "rel_expand_sum", "rel_contract_sum"]


def _as3(x):
    """[n], [n,F] or [n,H,D] -> [n,H,D] view."""
    if x.dim() == 1:
        return x.view(-1, 1, 1)
    if x.dim() == 2:
        return x.unsqueeze(1)
    if x.dim() == 3:
        return x
    return _flat2(x).unsqueeze(1)


def _flat2(t):
    """[n, ...] -> [n, prod(rest)] with an explicit width (n may be 0)."""
    w = 1
    for s in t.shape[1:]:
        w *= int(s)
    return t.reshape(t.shape[0], w)


def _edge2(a, H=None):
    """[E,H,1] / [E,H] / [E] -> [E,H]  (explicit width: E may be 0)."""
    w = 1
    for s in a.shape[1:]:
        w *= int(s)
    return a.reshape(a.shape[0], w)


def _pad4(x2):
    """[n,F] -> [n,F'] with F' the next multiple of 4 (zero columns): odd widths such as 41 classes would otherwise force
    4-byte lanes and one row per wavefront; padded they run with 16-byte lanes and several rows per wavefront."""
    F = x2.shape[1]
    return x2 if F % 4 == 0 or F < 5 else torch.nn.functional.pad(x2, (0, 4 - F % 4))


class _CopyUSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, x):
        ctx.g, ctx.shape = g, x.shape
        if x.dim() == 2:
            F = x.shape[1]
            out = _C.spmm(g.csc, _as3(_pad4(x)))
            return out.view(out.shape[0], -1)[:, :F].contiguous() if out.shape[2] != F else out.view(out.shape[0], F)
        return _C.spmm(g.csc, _as3(x)).view((g.number_of_dst_nodes(),) + tuple(x.shape[1:]))

    @staticmethod
    def backward(ctx, dout):
        g = ctx.g
        if len(ctx.shape) == 2:
            F = ctx.shape[1]
            dx = _C.spmm(g.csr, _as3(_pad4(dout.contiguous())))
            return None, (dx.view(dx.shape[0], -1)[:, :F].contiguous() if dx.shape[2] != F else dx.view(ctx.shape))
        return None, _C.spmm(g.csr, _as3(dout.contiguous())).view(ctx.shape)


def copy_u_sum(g, x):
    """`update_all(fn.copy_src('h','m'), fn.sum('m','h'))` — models.py:374,381."""
    return _CopyUSum.apply(g, x)


class _CopyUMax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, x, relu):
        if x.dim() not in (2, 3):
            raise ValueError(f"copy_u_max takes [n_src, F] or [n_src, H, D] features, got {tuple(x.shape)}")
        if x.shape[0] != g.number_of_src_nodes():
            raise ValueError(f"copy_u_max takes features of the graph's {g.number_of_src_nodes()} source nodes, got {x.shape[0]} rows")
        x2 = _flat2(x)
        F = x2.shape[1]
        out, arg = _C.spmm_max(g.csc, _pad4(x2), relu)
        ctx.g, ctx.shape, ctx.F = g, x.shape, F
        ctx.save_for_backward(arg)
        if out.shape[1] != F:           # the padded zero columns are sliced off
            out, arg = out[:, :F].contiguous(), arg[:, :F].contiguous()
        tail = tuple(x.shape[1:])
        out, arg = out.view((out.shape[0],) + tail), arg.view((arg.shape[0],) + tail)
        ctx.mark_non_differentiable(arg)
        return out, arg

    @staticmethod
    def backward(ctx, dout, _darg):
        g, F = ctx.g, ctx.F
        arg, = ctx.saved_tensors
        d2 = _pad4(_flat2(dout).contiguous())
        dx = _C.spmm_max_bwd(g.csr, g.csr2csc, d2, arg)      # the CSR is built here: only when a gradient is asked for
        if dx.shape[1] != F:
            dx = dx[:, :F].contiguous()
        return None, dx.view(ctx.shape), None


def copy_u_max(g, x, relu=False, return_arg=False):
    """`update_all(fn.copy_u('h','m'), fn.max('m','h'))`: out[v] = the element-wise max of x[u] over the in-edges u -> v; a destination
    without in-edges gets 0.  x: [n_src, F] or [n_src, H, D].  relu=True: `max(out, 0)`, i.e. the max over relu(x) without a ReLU pass over
    [n_src, F] (GraphSAGE's pool aggregator).  The gradient goes to ONE in-edge per (destination, column): the earliest one in the CSC
    that attains the max (none where relu gated it, or the row is empty).  return_arg: also that edge's CSC position (int32, the
    shape of out, -1 for none), non-differentiable."""
    out, arg = _CopyUMax.apply(g, x, bool(relu))
    return (out, arg) if return_arg else out


PNA_IMPLS = ("kernel", "tensor")
pna_default_impl = "kernel"              # for GPU tensors (README "PNA"); CPU tensors take "tensor"
pna_edge_default_impl = "kernel"         # `pna_aggregate_edge` on GPU tensors (README "PNA with edge features")
PNA_AGGREGATORS = ("mean", "sum", "max", "min", "std", "var")
PNA_SCALERS = ("identity", "amplification", "attenuation")


def _pna_impl(impl, t):
    """The form one call runs: the argument, else the BOT_PNA variable (read at call time), else the default for the device."""
    if impl is None:
        impl = os.environ.get("BOT_PNA") or (pna_default_impl if t.is_cuda else "tensor")
    if impl not in PNA_IMPLS:
        raise ValueError(f"pna_aggregate: impl (or BOT_PNA) must be one of {PNA_IMPLS}, got {impl!r}")
    return impl


def pna_check_names(aggregators, scalers):
    """DGL's names, checked: (aggregators, scalers) as tuples.  moment3 / moment4 / moment5 are not built (NotImplementedError); an
    unknown name raises DGLError."""
    from .errors import DGLError
    aggregators, scalers = tuple(aggregators), tuple(scalers)
    for a in aggregators:
        if a in ("moment3", "moment4", "moment5"):
            raise NotImplementedError(f"PNA: the {a} aggregator is not built (DESIGN §8); use {PNA_AGGREGATORS}")
        if a not in PNA_AGGREGATORS:
            raise DGLError(f"PNA: unknown aggregator {a!r}; one of {PNA_AGGREGATORS}")
    for sc in scalers:
        if sc not in PNA_SCALERS:
            raise DGLError(f"PNA: unknown scaler {sc!r}; one of {PNA_SCALERS}")
    if not aggregators or not scalers or len(aggregators) > 8 or len(scalers) > 8:
        raise DGLError("PNA: 1 .. 8 aggregators and 1 .. 8 scalers")
    return aggregators, scalers


def pna_scale_table(g, scalers, delta):
    """float32 [S, n_dst], row s = scaler s of every destination's in-degree n: identity 1, amplification log(n + 1) / delta,
    attenuation delta / log(n + 1); 0 for a destination without in-edges (its output row is 0 whatever the scaler).  Built once per
    (graph, scalers, delta)."""
    from .nn import _graph_cache
    c = _graph_cache(g)
    key = ("pna_scale", tuple(scalers), float(delta))
    if key not in c:
        deg = g.in_degrees()
        L = torch.log(deg.to(torch.float32) + 1.0)
        one, zero = torch.ones_like(L), torch.zeros_like(L)
        rows = {"identity": one, "amplification": L / float(delta), "attenuation": float(delta) / torch.where(deg > 0, L, one)}
        c[key] = torch.stack([torch.where(deg > 0, rows[s], zero) for s in scalers]).contiguous()
    return c[key]


def _pna_layout(vals, scale, Ft):
    """[n, A, F] aggregator values and the [S, n] scalers -> [n, S*A*F] tower-major: column tower * S*A*Ft + (s*A + a) * Ft + f."""
    n, A, F = vals.shape
    S = scale.shape[0]
    v = vals.reshape(n, 1, A, F // Ft, Ft) * scale.t().reshape(n, S, 1, 1, 1)
    return v.permute(0, 3, 1, 2, 4).reshape(n, S * A * F)


def _pna_tensor(g, a, b, aggregators, scale, Ft):
    """The composition from the existing sweeps: two sum sweeps (a, a * a) and two max sweeps (a, -a), then dense tensor ops."""
    deg = g.in_degrees()
    some = (deg > 0).reshape(-1, 1)
    n = deg.to(a.dtype).clamp(min=1).reshape(-1, 1)
    zero = torch.zeros((), dtype=a.dtype, device=a.device)
    kinds = set(aggregators)
    bb = zero if b is None else b
    val, saved, sarg = {}, None, None
    s1 = copy_u_sum(g, a)
    mean_a = s1 / n
    if "mean" in kinds:
        val["mean"] = mean_a + bb
    if "sum" in kinds:
        val["sum"] = s1 + n * bb
    neg1 = torch.full((g.number_of_dst_nodes(), a.shape[1]), -1, dtype=torch.int32, device=a.device)
    amax = amin = neg1
    if "max" in kinds:
        m, amax = copy_u_max(g, a, return_arg=True)
        val["max"] = m + bb
    if "min" in kinds:
        m, amin = copy_u_max(g, -a, return_arg=True)
        val["min"] = bb - m
    gate = torch.zeros_like(mean_a)
    if kinds & {"std", "var"}:
        var = torch.relu(copy_u_sum(g, a * a) / n - mean_a * mean_a)
        std = torch.sqrt(var + 1e-30)
        val["var"], val["std"] = var, std
        gate = torch.where(var > 0, std, zero).detach()
    vals = torch.stack([torch.where(some, val[k], zero) for k in aggregators], dim=1)
    saved = torch.cat([torch.where(some, mean_a.detach(), zero), torch.where(some, gate, zero)], dim=1)
    sarg = torch.cat([amax, amin], dim=1)
    return _pna_layout(vals, scale, Ft), saved, sarg


class _PNAAggregate(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, a, b, aggregators, scale, Ft, want_saved):
        need = want_saved or ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        out, saved, sarg = _C.spmm_pna(g.csc, a, b, aggregators, scale, Ft, want_saved=need)
        ctx.g, ctx.aggregators, ctx.scale, ctx.Ft, ctx.has_b = g, aggregators, scale, Ft, b is not None
        if need:
            ctx.save_for_backward(a, saved, sarg)
            ctx.mark_non_differentiable(saved, sarg)
        return out, saved, sarg

    @staticmethod
    def backward(ctx, dout, _ds, _dg):
        g = ctx.g
        a, saved, sarg = ctx.saved_tensors
        want_db = ctx.has_b and ctx.needs_input_grad[2]
        rec, db = _C.pna_bwd_prep(g.csc, dout.contiguous(), ctx.aggregators, saved, sarg, ctx.scale, ctx.Ft, want_db=want_db)
        da = None
        if ctx.needs_input_grad[1]:         # the CSR is built here: only when the gradient of a is asked for
            da = _C.spmm_pna_bwd(g.csr, g.csr2csc, a, rec, ctx.aggregators)
        return None, da, db, None, None, None, None


def pna_aggregate(g, a, b=None, aggregators=("mean", "max", "min", "std"), scalers=("identity", "amplification", "attenuation"), delta=1.0,
                  tower_width=None, impl=None, return_saved=False):
    """Principal Neighbourhood Aggregation (Corso et al., NeurIPS 2020) of the messages m = a[u] + b[v] over the in-edges
    u -> v: per destination and column the chosen `aggregators` ("mean", "sum", "max", "min", "std", "var";
    var = relu(mean m^2 - mean(m)^2), std = sqrt(var + 1e-30)), each times the `scalers` of the in-degree n ("identity",
    "amplification" log(n + 1) / delta, "attenuation" delta / log(n + 1)).  a: float32 [n_src, F]; b: float32 [n_dst, F] or None.
    Returns [n_dst, S*A*F]: towers of `tower_width` = Ft columns (default one tower of F) one after the other, inside a tower block
    (s, a) at column (s*A + a) * Ft.  A destination without in-edges gets a zero row (no b).  Gradients flow to a and b; max and min
    send theirs to the smallest CSC position that attains them, std has gradient 0 where var == 0.  impl: "kernel" (one fused sweep,
    csrc/spmm_pna.hip; GPU tensors) or "tensor" (sum sweeps over a and a * a, max sweeps over a and -a; what CPU tensors take).
    return_saved: also (saved float32 [n_dst, 2F] = the mean of a | std where var > 0 else 0, sarg int32 [n_dst, 2F] = the positions of
    the max | of the min, -1 where there is none), non-differentiable."""
    aggregators, scalers = pna_check_names(aggregators, scalers)
    if a.dim() != 2 or a.shape[0] != g.number_of_src_nodes():
        raise ValueError(f"pna_aggregate takes a [n_src = {g.number_of_src_nodes()}, F], got {tuple(a.shape)}")
    F = int(a.shape[1])
    if b is not None and tuple(b.shape) != (g.number_of_dst_nodes(), F):
        raise ValueError(f"pna_aggregate takes b [n_dst = {g.number_of_dst_nodes()}, {F}], got {tuple(b.shape)}")
    Ft = F if tower_width is None else int(tower_width)
    if Ft < 1 or F % Ft:
        raise ValueError(f"pna_aggregate: tower_width {Ft} does not divide F = {F}")
    scale = pna_scale_table(g, scalers, delta)
    if _pna_impl(impl, a) == "tensor":
        out, saved, sarg = _pna_tensor(g, a, b, aggregators, scale, Ft)
    else:
        if a.shape[1] > 1 and a.stride(1) != 1:
            a = a.contiguous()
        if b is not None and b.shape[1] > 1 and b.stride(1) != 1:
            b = b.contiguous()
        out, saved, sarg = _PNAAggregate.apply(g, a, b, aggregators, scale, Ft, bool(return_saved))
    return (out, saved, sarg) if return_saved else out


def _take_rows_grad(x, idx):
    """`take_rows` that carries a gradient at any length: above its piece size `take_rows` fills one buffer piece by piece, which
    autograd cannot follow, so a tensor that requires a gradient is gathered piece by piece and concatenated."""
    if idx.numel() <= _TAKE_CHUNK or not (x.requires_grad and torch.is_grad_enabled()):
        return take_rows(x, idx)
    idx = idx.long()
    return torch.cat([x[idx[i:i + _TAKE_CHUNK]] for i in range(0, idx.numel(), _TAKE_CHUNK)])


def _pna_edge_tensor(g, a, b, ef, weight, aggregators, scale, Ft):
    """The tensor form of `pna_aggregate_edge`: per-position messages [E, F], segment sums, a two-pass variance; the extremes and their
    owners are the smallest position that equals the extreme."""
    n_dst, F, E = g.number_of_dst_nodes(), a.shape[1], g.number_of_edges()
    deg = g.in_degrees()
    some = (deg > 0).reshape(-1, 1)
    n = deg.to(a.dtype).clamp(min=1).reshape(-1, 1)
    zero = torch.zeros((), dtype=a.dtype, device=a.device)
    kinds = set(aggregators)
    bb = zero if b is None else b
    rows = _csc_edge_rows(g)
    m = _take_rows_grad(a, g.csc.indices) + (ef if rows is None else _take_rows_grad(ef, rows)) @ weight.t()          # [E, F], CSC position order
    seg = csc_destinations(g)
    s1 = _segment_sum_positions(g, m)
    mean_m = s1 / n
    val = {"mean": mean_m + bb, "sum": s1 + n * bb}
    neg1 = torch.full((n_dst, F), -1, dtype=torch.int32, device=a.device)
    pos = torch.arange(E, dtype=torch.int64, device=a.device).reshape(-1, 1).expand(-1, F)
    segs = seg.long().reshape(-1, 1).expand(-1, F)

    def extreme(kind):
        md = m.detach()
        ext = torch.zeros((n_dst, F), dtype=a.dtype, device=a.device).scatter_reduce(0, segs, md, kind, include_self=False)
        hit = torch.where(md == take_rows(ext, seg), pos, torch.full_like(pos, E))
        own = torch.full((n_dst, F), E, dtype=torch.int64, device=a.device).scatter_reduce(0, segs, hit, "amin", include_self=True)
        own = torch.where(own < E, own, torch.full_like(own, -1))      # an empty row, or a row whose extreme is a NaN: no owner
        v = torch.where(own >= 0, m.gather(0, own.clamp(min=0)), zero)
        return v, own.to(torch.int32)
    amax = amin = neg1
    if "max" in kinds:
        v, amax = extreme("amax")
        val["max"] = v + bb
    if "min" in kinds:
        v, amin = extreme("amin")
        val["min"] = v + bb
    gate = torch.zeros_like(mean_m)
    if kinds & {"std", "var"}:
        dev2 = m - _take_rows_grad(mean_m, seg)
        var = torch.relu(_segment_sum_positions(g, dev2 * dev2) / n)
        std = torch.sqrt(var + 1e-30)
        val["var"], val["std"] = var, std
        gate = torch.where(var > 0, std, zero).detach()
    vals = torch.stack([torch.where(some, val[k], zero) for k in aggregators], dim=1)
    saved = torch.cat([torch.where(some, mean_m.detach(), zero), torch.where(some, gate, zero)], dim=1)
    sarg = torch.cat([amax, amin], dim=1)
    return _pna_layout(vals, scale, Ft), saved, sarg


class _PNAAggregateEdge(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, a, b, ef, weight, aggregators, scale, Ft, want_saved):
        need = want_saved or any(ctx.needs_input_grad[i] for i in (1, 2, 4))
        ef, wd = ef.contiguous(), weight.detach()
        out, saved, sarg = _C.spmm_pna_edge(g.csc, a, b, ef, wd, aggregators, scale, Ft, want_saved=need, eperm=_csc_edge_rows(g))
        ctx.g, ctx.aggregators, ctx.scale, ctx.Ft, ctx.has_b = g, aggregators, scale, Ft, b is not None
        if need:
            ctx.save_for_backward(a, ef, wd, saved, sarg)
            ctx.mark_non_differentiable(saved, sarg)
        return out, saved, sarg

    @staticmethod
    def backward(ctx, dout, _ds, _dg):
        g = ctx.g
        a, ef, wd, saved, sarg = ctx.saved_tensors
        need_a, need_w = ctx.needs_input_grad[1], ctx.needs_input_grad[4]
        want_db = ctx.has_b and ctx.needs_input_grad[2]
        rec, db = _C.pna_bwd_prep(g.csc, dout.contiguous(), ctx.aggregators, saved, sarg, ctx.scale, ctx.Ft, want_db=want_db)
        da = dweight = None
        if need_a or need_w:                # the CSR is built here: only when the gradient of a or of weight is asked for
            da, dweight = _C.spmm_pna_edge_bwd(g.csr, g.csr2csc, a, ef, wd, rec, ctx.aggregators, eperm=g.csr.eid, want_dx=need_a,
                                               want_dweight=need_w)
        return None, da, db, None, dweight, None, None, None, None


def pna_aggregate_edge(g, a, b, ef, weight, aggregators=("mean", "max", "min", "std"), scalers=("identity", "amplification", "attenuation"),
                       delta=1.0, tower_width=None, impl=None, return_saved=False):
    """`pna_aggregate` over per-EDGE messages whose edge term is a projection of K raw edge features, formed inside the sweep (DGL's
    `PNAConv(edge_feat_size=K)`, whose pretrans M(cat[h_u, h_v, e_uv]) is linear):

        m_e = a[u] + ef[e] @ weight.T  (+ b[v] behind the reduce)   for the edge e = u -> v: the sum over j = 0 .. K-1 in index order

    a: float32 [n_src, F]; b: float32 [n_dst, F] or None; ef: [E, K] in EDGE-ID order (on a Block or Subgraph that is the CSC position);
    weight: [F, K], as `nn.Linear(K, F)` stores it.  Returns `pna_aggregate`'s layout (and, with return_saved, saved = the mean of the
    messages without b | the std gate, sarg = the owner positions of max | min).  Gradients: a, b and weight; `ef` gets none from the
    kernel form.  impl="kernel" (float32): one sweep over the CSC that reads the K floats of an edge beside its source row, the moments
    around a split pivot (a and the edge term apart), and one persistent sweep over the CSR that forms the edge term again per out-edge
    for da and dweight (csrc/spmm_pna_edge.hip); nothing of size [E, F] exists, no float atomics.  impl="tensor": per-position messages
    take_rows(a, indices) + ef_pos @ weight.T, segment sums, a two-pass variance, the extremes owned by the smallest position that
    equals them: what CPU tensors run, what the kernel form falls back to when K > 16 or `ef` requires a gradient, and what the kernels
    are timed against.  impl=None: the BOT_PNA variable, else `pna_edge_default_impl` on the GPU.  A graph with a halo plan raises
    ValueError."""
    if g.halo is not None:
        raise ValueError("pna_aggregate_edge on a partitioned graph (a halo plan) is not supported: it takes whole graphs, Subgraphs and "
                         "sampled blocks")
    aggregators, scalers = pna_check_names(aggregators, scalers)
    if a.dim() != 2:
        raise ValueError(f"pna_aggregate_edge takes [n_src, F] features, got {tuple(a.shape)}")
    if a.shape[0] != g.number_of_src_nodes():
        raise ValueError(f"pna_aggregate_edge takes features of the graph's {g.number_of_src_nodes()} source nodes, got {a.shape[0]} rows")
    E, F = g.number_of_edges(), int(a.shape[1])
    if b is not None and tuple(b.shape) != (g.number_of_dst_nodes(), F):
        raise ValueError(f"pna_aggregate_edge takes b [n_dst = {g.number_of_dst_nodes()}, {F}], got {tuple(b.shape)}")
    if ef is None or ef.dim() != 2 or ef.shape[0] != E or ef.shape[1] < 1:
        raise ValueError(f"pna_aggregate_edge: ef must be [{E}, K >= 1] (one row per edge, edge-id order), got "
                         f"{None if ef is None else tuple(ef.shape)}")
    K = int(ef.shape[1])
    if tuple(weight.shape) != (F, K):
        raise ValueError(f"pna_aggregate_edge: weight must be [{F}, {K}] (as nn.Linear({K}, {F}) stores it), got {tuple(weight.shape)}")
    for name, t in (("b", b), ("ef", ef), ("weight", weight)):
        if t is not None and (t.dtype != a.dtype or t.device != a.device):
            raise ValueError(f"pna_aggregate_edge: {name} must be {a.dtype} on {a.device} like a, got {t.dtype} on {t.device}")
    Ft = F if tower_width is None else int(tower_width)
    if Ft < 1 or F % Ft:
        raise ValueError(f"pna_aggregate_edge: tower_width {Ft} does not divide F = {F}")
    if impl is None:
        impl = os.environ.get("BOT_PNA") or (pna_edge_default_impl if a.is_cuda else "tensor")
    if impl not in PNA_IMPLS:
        raise ValueError(f"pna_aggregate_edge: impl (or BOT_PNA) must be one of {PNA_IMPLS}, got {impl!r}")
    scale = pna_scale_table(g, scalers, delta)
    grad = torch.is_grad_enabled()
    if impl == "kernel" and a.dtype == torch.float32 and K <= _C.PNA_EDGE_MAX_K and not (ef.requires_grad and grad):
        if a.shape[1] > 1 and a.stride(1) != 1:
            a = a.contiguous()
        if b is not None and b.shape[1] > 1 and b.stride(1) != 1:
            b = b.contiguous()
        out, saved, sarg = _PNAAggregateEdge.apply(g, a, b, ef, weight, aggregators, scale, Ft, bool(return_saved))
    else:
        out, saved, sarg = _pna_edge_tensor(g, a, b, ef, weight, aggregators, scale, Ft)
    return (out, saved, sarg) if return_saved else out


def copy_u_min(g, x, impl=None):
    """`update_all(fn.copy_u('h','m'), fn.min('m','h'))`: out[v] = the element-wise min of x[u] over the in-edges u -> v; a destination
    without in-edges gets 0.  x: [n_src, F] or [n_src, H, D].  The PNA sweep with one aggregator and no scaler; the gradient goes to the
    earliest CSC position that attains the min.  CPU tensors (impl="tensor") take -copy_u_max(-x)."""
    if x.dim() not in (2, 3):
        raise ValueError(f"copy_u_min takes [n_src, F] or [n_src, H, D] features, got {tuple(x.shape)}")
    if x.shape[0] != g.number_of_src_nodes():
        raise ValueError(f"copy_u_min takes features of the graph's {g.number_of_src_nodes()} source nodes, got {x.shape[0]} rows")
    if _pna_impl(impl, x) == "tensor":
        return -copy_u_max(g, -x)
    x2 = _flat2(x)
    if x2.shape[1] > 1 and x2.stride(1) != 1:
        x2 = x2.contiguous()
    out, _, _ = _PNAAggregate.apply(g, x2, None, ("min",), None, x2.shape[1], False)
    return out.view((out.shape[0],) + tuple(x.shape[1:]))


SOFTMAX_AGG_IMPLS = ("kernel", "tensor")
softmax_agg_default_impl = "kernel"      # for GPU tensors (README "DeeperGCN / softmax aggregation"); CPU tensors take "tensor"
_BETA_CACHE = {}                         # (device, value) -> the one-element float32 tensor the kernels read a Python-float beta from
_BETA_CACHE_MAX = 64                     # entries; a caller that sweeps beta passes a tensor, or pays one small copy per new value


def _softmax_agg_impl(impl, t, who="copy_u_softmax"):
    """The form one call runs: the argument, else the BOT_SOFTMAX_AGG variable (read at call time), else the default for the device."""
    if impl is None:
        impl = os.environ.get("BOT_SOFTMAX_AGG") or (softmax_agg_default_impl if t.is_cuda else "tensor")
    if impl not in SOFTMAX_AGG_IMPLS:
        raise ValueError(f"{who}: impl (or BOT_SOFTMAX_AGG) must be one of {SOFTMAX_AGG_IMPLS}, got {impl!r}")
    return impl


def _device_beta(beta, like):
    """A Python-float beta as a one-element float32 tensor on `like`'s device: placed there once per (device, value)."""
    key = (like.device, float(beta))
    if key not in _BETA_CACHE:
        if len(_BETA_CACHE) >= _BETA_CACHE_MAX:        # bounded: dropped whole rather than grown without end
            _BETA_CACHE.clear()
        _BETA_CACHE[key] = torch.full((1,), float(beta), dtype=torch.float32, device=like.device)
    return _BETA_CACHE[key]


def softmax_agg_positions(g, msg, beta):
    """The tensor form of the softmax aggregation over per-POSITION messages: msg [E, F] in CSC position order (row k is the message
    of the in-edge at position k), beta a float or a one-element tensor -> out [n_dst, F] = sum_k softmax_k(beta msg_k) msg_k per
    destination and column, 0 for a destination without in-edges.  A segment max, an exp and two segment sums in torch ops,
    differentiable in msg and beta; it materialises [E, F]."""
    n_dst, E = g.number_of_dst_nodes(), msg.shape[0]
    deg = (g.csc.indptr[1:] - g.csc.indptr[:-1]).long()
    seg = torch.repeat_interleave(torch.arange(n_dst, device=msg.device), deg, output_size=E)
    b = msg * beta
    zeros = torch.zeros((n_dst, msg.shape[1]), dtype=msg.dtype, device=msg.device)
    mx = zeros.scatter_reduce(0, seg.reshape(-1, 1).expand(-1, msg.shape[1]), b.detach(), "amax", include_self=False)
    e = torch.exp(b - mx[seg])                      # the shift is a constant of the softmax: detached
    Z = zeros.index_add(0, seg, e)
    S = zeros.index_add(0, seg, e * msg)
    return S / torch.where((deg > 0).reshape(-1, 1), Z, torch.ones((), dtype=msg.dtype, device=msg.device))   # an empty row: 0 / 1


class _CopyUSoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, x, beta, relu, eps, want_q):
        x2 = _pad4(_flat2(x))
        out, lse, q = _C.spmm_softmax(g.csc, x2, beta.detach(), relu, eps, want_q)
        ctx.g, ctx.shape, ctx.F, ctx.relu, ctx.eps = g, x.shape, _flat2(x).shape[1], relu, eps
        ctx.save_for_backward(x2, beta, out, lse, q)
        if out.shape[1] != ctx.F:           # the padded zero columns are sliced off
            out = out[:, :ctx.F].contiguous()
        return out.view((out.shape[0],) + tuple(x.shape[1:]))

    @staticmethod
    def backward(ctx, dout):
        g, F = ctx.g, ctx.F
        x2, beta, out, lse, q = ctx.saved_tensors
        d2 = _pad4(_flat2(dout).contiguous())
        dx = dbeta = None
        if ctx.needs_input_grad[1]:         # the CSR is built here: only when the features' gradient is asked for
            dx = _C.spmm_softmax_bwd(g.csr, x2, beta.detach(), ctx.relu, ctx.eps, d2, out, lse)
            if dx.shape[1] != F:
                dx = dx[:, :F].contiguous()
            dx = dx.view(ctx.shape)
        if ctx.needs_input_grad[2]:         # d out / d beta = q - out^2: a dense reduction, accumulated in float64
            dbeta = torch.sum(d2 * torch.addcmul(q, out, out, value=-1.0), dtype=torch.float64).to(beta.dtype).reshape(beta.shape)
        return None, dx, dbeta, None, None, None


def copy_u_softmax(g, x, beta=1.0, relu=False, eps=0.0, impl=None):
    """The per-channel softmax aggregation of DeeperGCN (Li et al., arXiv:2006.07739; DGL's / PyG's GENConv, PyG's SoftmaxAggregation):

        m_u = relu ? max(x[u], 0) + eps : x[u];   out[v, f] = sum over the in-edges u -> v of softmax_u(beta m_u[f]) m_u[f]

    x: [n_src, F] or [n_src, H, D]; a destination without in-edges gets 0.  A NaN in x stays a NaN in the rows that gather it, in both
    forms.  beta: a Python float (placed on the device once per value; at most 64 values are kept) or
    a one-element float32 tensor / parameter, which the kernels read from device memory; its gradient is the weighted variance of the
    messages.  The derivative of the ReLU at 0 is 0 (torch's convention).  impl="kernel": one online-softmax sweep over the CSC and one
    sweep over the CSR for the gradient (csrc/spmm_softmax.hip; the CSR is built only when x needs a gradient); nothing of size [E, F]
    exists.  impl="tensor": a gather to [E, F], a segment max, exp and two segment sums in torch ops: what runs on CPU tensors and what
    the kernels are timed against.  impl=None: the BOT_SOFTMAX_AGG variable, else `softmax_agg_default_impl` on the GPU.  Whole graphs,
    Subgraphs and sampled blocks; a graph with a halo plan raises ValueError."""
    if g.halo is not None:
        raise ValueError("copy_u_softmax on a partitioned graph (a halo plan) is not supported: it takes whole graphs, Subgraphs and "
                         "sampled blocks")
    if x.dim() not in (2, 3):
        raise ValueError(f"copy_u_softmax takes [n_src, F] or [n_src, H, D] features, got {tuple(x.shape)}")
    if x.shape[0] != g.number_of_src_nodes():
        raise ValueError(f"copy_u_softmax takes features of the graph's {g.number_of_src_nodes()} source nodes, got {x.shape[0]} rows")
    if isinstance(beta, torch.Tensor):
        if beta.numel() != 1 or beta.dtype != x.dtype or beta.device != x.device:
            raise ValueError(f"copy_u_softmax: a tensor beta holds one {x.dtype} on {x.device}, got {tuple(beta.shape)} {beta.dtype} on "
                             f"{beta.device}")
    if _softmax_agg_impl(impl, x) == "kernel":
        bt = beta if isinstance(beta, torch.Tensor) else _device_beta(beta, x)
        want_q = bt.requires_grad and torch.is_grad_enabled()          # q is the saved statistic of beta's gradient: only when one can be asked for
        return _CopyUSoftmax.apply(g, x, bt, bool(relu), float(eps), want_q)
    m = take_rows(_flat2(x), g.csc.indices)
    if relu:
        m = torch.relu(m) + eps
    out = softmax_agg_positions(g, m, beta.reshape(()) if isinstance(beta, torch.Tensor) else float(beta))
    return out.view((out.shape[0],) + tuple(x.shape[1:]))


def _csc_edge_rows(g):
    """The row of an edge-id-ordered edge tensor for every CSC position, or None where it is the position itself (batch graphs)."""
    from .sampling import _BatchGraph
    return None if isinstance(g, _BatchGraph) else g.csc.eid


class _UAddESoftmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, x, ef, weight, bias, beta, relu, eps, want_q):
        x2 = x if x.stride(1) == 1 or x.shape[1] == 1 else x.contiguous()
        ef, wd = ef.contiguous(), weight.detach()
        bd = None if bias is None else bias.detach().contiguous()
        out, lse, q = _C.spmm_softmax_edge(g.csc, x2, ef, wd, bd, beta.detach(), relu, eps, want_q, eperm=_csc_edge_rows(g))
        ctx.g, ctx.relu, ctx.eps, ctx.has_bias = g, relu, eps, bias is not None
        ctx.save_for_backward(x2, ef, wd, bd, beta, out, lse, q)
        return out

    @staticmethod
    def backward(ctx, dout):
        g = ctx.g
        x2, ef, wd, bd, beta, out, lse, q = ctx.saved_tensors
        need_x, need_w, need_b, need_beta = (ctx.needs_input_grad[i] for i in (1, 3, 4, 5))
        need_b = need_b and ctx.has_bias
        d2 = dout.contiguous()
        dx = dweight = dbias = dbeta = None
        if need_x or need_w or need_b:      # the CSR is built here: only when a gradient is asked for.  dbias is the column sum of dx.
            dx, dweight = _C.spmm_softmax_edge_bwd(g.csr, x2, ef, wd, bd, beta.detach(), ctx.relu, ctx.eps, d2, out, lse, eperm=g.csr.eid,
                                                   want_dx=need_x or need_b, want_dweight=need_w)
            if need_b:                      # a dense column reduction, accumulated in float64
                dbias = torch.sum(dx, dim=0, dtype=torch.float64).to(dx.dtype)
            if not need_x:
                dx = None
        if need_beta:                       # d out / d beta = q - out^2, as in copy_u_softmax
            dbeta = torch.sum(d2 * torch.addcmul(q, out, out, value=-1.0), dtype=torch.float64).to(beta.dtype).reshape(beta.shape)
        return None, dx, None, dweight, dbias, dbeta, None, None, None


def u_add_e_softmax(g, x, ef, weight, bias=None, beta=1.0, relu=False, eps=0.0, impl=None):
    """The softmax aggregation of `copy_u_softmax` over per-EDGE messages whose edge term is a projection of K raw edge features
    (DeeperGCN's GENConv with an edge encoder, PyG's `GENConv(edge_dim=K)`), formed inside the sweep:

        z_e = x[u] + (ef[e] @ weight.T + bias)   for the edge e = u -> v: the sum over j = 0 .. K-1 in index order, then the bias, then x
        m_e = relu ? max(z_e, 0) + eps : z_e;    out[v, f] = sum over the in-edges e of v of softmax_e(beta m_e[f]) m_e[f]

    x: [n_src, F]; ef: [E, K] in EDGE-ID order (on a Block or Subgraph that is the CSC position); weight: [F, K], as `nn.Linear(K, F)` stores
    it; bias: [F] or None; beta, relu, eps as in `copy_u_softmax`.  Gradients: x, weight, bias and a tensor beta; `ef` gets none from the
    kernel form.  impl="kernel" (float32): one sweep over the CSC that reads the K floats of an edge beside its source row and one
    persistent sweep over the CSR that recomputes z per out-edge for dx and dweight (csrc/spmm_softmax_edge.hip); dbias is the column sum
    of dx; nothing of size [E, F] exists, no float atomics.  impl="tensor": relu(take_rows(x, indices) + ef_pos @ weight.T + bias) + eps
    followed by `softmax_agg_positions`: what CPU tensors run, what the kernel form falls back to when K > 16 or `ef` requires a
    gradient, and what the kernels are timed against.  impl=None: the BOT_SOFTMAX_AGG variable, else `softmax_agg_default_impl` on the
    GPU.  A graph with a halo plan raises ValueError."""
    if g.halo is not None:
        raise ValueError("u_add_e_softmax on a partitioned graph (a halo plan) is not supported: it takes whole graphs, Subgraphs and "
                         "sampled blocks")
    if x.dim() != 2:
        raise ValueError(f"u_add_e_softmax takes [n_src, F] features, got {tuple(x.shape)}")
    if x.shape[0] != g.number_of_src_nodes():
        raise ValueError(f"u_add_e_softmax takes features of the graph's {g.number_of_src_nodes()} source nodes, got {x.shape[0]} rows")
    E, F = g.number_of_edges(), int(x.shape[1])
    if ef.dim() != 2 or ef.shape[0] != E or ef.shape[1] < 1:
        raise ValueError(f"u_add_e_softmax: ef must be [{E}, K >= 1] (one row per edge, edge-id order), got {tuple(ef.shape)}")
    K = int(ef.shape[1])
    if tuple(weight.shape) != (F, K):
        raise ValueError(f"u_add_e_softmax: weight must be [{F}, {K}] (as nn.Linear({K}, {F}) stores it), got {tuple(weight.shape)}")
    if bias is not None and tuple(bias.shape) != (F,):
        raise ValueError(f"u_add_e_softmax: bias must be [{F}], got {tuple(bias.shape)}")
    for name, t in (("ef", ef), ("weight", weight), ("bias", bias)):
        if t is not None and (t.dtype != x.dtype or t.device != x.device):
            raise ValueError(f"u_add_e_softmax: {name} must be {x.dtype} on {x.device} like x, got {t.dtype} on {t.device}")
    if isinstance(beta, torch.Tensor):
        if beta.numel() != 1 or beta.dtype != x.dtype or beta.device != x.device:
            raise ValueError(f"u_add_e_softmax: a tensor beta holds one {x.dtype} on {x.device}, got {tuple(beta.shape)} {beta.dtype} on "
                             f"{beta.device}")
    grad = torch.is_grad_enabled()
    if _softmax_agg_impl(impl, x, "u_add_e_softmax") == "kernel" and K <= _C.SOFTMAX_EDGE_MAX_K and not (ef.requires_grad and grad):
        bt = beta if isinstance(beta, torch.Tensor) else _device_beta(beta, x)
        return _UAddESoftmax.apply(g, x, ef, weight, bias, bt, bool(relu), float(eps), bt.requires_grad and grad)
    rows = _csc_edge_rows(g)
    z = (ef if rows is None else take_rows(ef, rows)) @ weight.t()
    if bias is not None:
        z = z + bias
    m = take_rows(x, g.csc.indices) + z
    if relu:
        m = torch.relu(m) + eps
    return softmax_agg_positions(g, m, beta.reshape(()) if isinstance(beta, torch.Tensor) else float(beta))


GATV2_IMPLS = ("kernel", "tensor")
gatv2_default_impl = "kernel"      # for GPU tensors (README "GATv2": the kernel form against the tensor form); CPU tensors take "tensor"


def _gatv2_impl(impl, t):
    """The form one call runs: the argument, else the BOT_GATV2 variable (read at call time), else the default for the tensor's device."""
    if impl is None:
        impl = os.environ.get("BOT_GATV2") or (gatv2_default_impl if t.is_cuda else "tensor")
    if impl not in GATV2_IMPLS:
        raise ValueError(f"gatv2_logits: impl (or BOT_GATV2) must be one of {GATV2_IMPLS}, got {impl!r}")
    return impl


class _GATv2Logits(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, fs, fd, attn, slope, order):
        csc = g.csc
        fs, fd, at = _rows_contiguous(fs), _rows_contiguous(fd), attn.reshape(attn.shape[-2:]).contiguous()
        e = _C.gatv2_logits(csc, fs, fd, at, slope, csc.eid if order == "eid" else None)
        ctx.g, ctx.slope, ctx.order, ctx.ashape = g, slope, order, attn.shape
        ctx.save_for_backward(fs, fd, at)
        return e.view(-1, at.shape[0], 1)

    @staticmethod
    def backward(ctx, de):
        g = ctx.g
        fs, fd, at = ctx.saved_tensors
        H = at.shape[0]
        de2 = de.reshape(-1, H).contiguous()
        eid = ctx.order == "eid"
        dfs = dfd = dattn = None
        if ctx.needs_input_grad[2] or ctx.needs_input_grad[3]:
            dfd, dattn = _C.gatv2_logits_bwd_dst(g.csc, fs, fd, at, ctx.slope, de2, g.csc.eid if eid else None,
                                                 want_dfd=ctx.needs_input_grad[2], want_dattn=ctx.needs_input_grad[3])
            if dattn is not None:
                dattn = dattn.view(ctx.ashape)
        if ctx.needs_input_grad[1]:         # the CSR is built here: only when the source rows' gradient is asked for
            csr = g.csr
            dfs = _C.gatv2_logits_bwd_src(csr, csr.eid if eid else g.csr2csc, fs, fd, at, ctx.slope, de2)
        return None, dfs, dfd, dattn, None, None


def _rows_contiguous(x):
    """[n, H, D] as the kernels take it: every row H * D contiguous floats (the row stride may be wider)."""
    H, D = x.shape[1], x.shape[2]
    ok = (D == 1 or x.stride(2) == 1) and (H == 1 or x.stride(1) == D) and (x.shape[0] <= 1 or x.stride(0) >= H * D)
    return x if ok else x.contiguous()


def gatv2_logits(g, fs, fd, attn, negative_slope=0.2, order="csc", impl=None):
    """The edge logits of GATv2 (Brody, Alon, Yahav, ICLR 2022; DGL's GATv2Conv):

        e[k, h] = sum_d attn[h, d] * leaky_relu(fs[u_k, h, d] + fd[v_k, h, d], negative_slope)

    fs: float32 [n_src, H, D]; fd: float32 [n_dst, H, D] (on a block n_dst < n_src); attn: [H, D] or [1, H, D].  Returns float32
    [E, H, 1] in CSC position order (order="csc", what `gat_attention(..., ee=e, ee_order="csc")` takes) or edge-id order ("eid").
    impl="kernel": one sweep that gathers the source row and reduces on the fly (csrc/gatv2.hip), with its two backward sweeps;
    nothing of size [E, H, D] exists.  impl="tensor": `u_add_v` -> `leaky_relu` -> `* attn` -> `.sum(-1)`, which materialises [E, H, D]:
    what runs on CPU tensors and what the kernels are timed against.  impl=None: the BOT_GATV2 variable, else `gatv2_default_impl` on
    the GPU.  The derivative of the leaky ReLU at 0 is negative_slope (torch's convention).  A graph with a halo plan raises ValueError."""
    if g.halo is not None:
        raise ValueError("gatv2_logits on a partitioned graph (a halo plan) is not supported: it takes whole graphs, Subgraphs and sampled blocks")
    if order not in ("csc", "eid"):
        raise ValueError(f'gatv2_logits: order must be "csc" or "eid", got {order!r}')
    if fs.dim() != 3 or fs.shape[0] != g.number_of_src_nodes():
        raise ValueError(f"gatv2_logits: fs must be [{g.number_of_src_nodes()}, H, D] (one row per source node), got {tuple(fs.shape)}")
    H, D = int(fs.shape[1]), int(fs.shape[2])
    if tuple(fd.shape) != (g.number_of_dst_nodes(), H, D):
        raise ValueError(f"gatv2_logits: fd must be [{g.number_of_dst_nodes()}, {H}, {D}] (one row per destination node), got {tuple(fd.shape)}")
    if tuple(attn.shape) not in ((H, D), (1, H, D)):
        raise ValueError(f"gatv2_logits: attn must be [{H}, {D}] or [1, {H}, {D}], got {tuple(attn.shape)}")
    if H < 1 or D < 1:
        raise ValueError(f"gatv2_logits: H and D must be at least 1, got fs {tuple(fs.shape)}")
    if _gatv2_impl(impl, fs) == "kernel":
        return _GATv2Logits.apply(g, fs, fd, attn, float(negative_slope), order)
    s = u_add_v(g, fs, fd)                                                     # [E, H, D], edge-id order
    e = (torch.nn.functional.leaky_relu(s, float(negative_slope)) * attn.reshape(1, H, D)).sum(-1, keepdim=True)
    return take_rows(e, g.csc.eid) if order == "csc" else e


GATE_IMPLS = ("kernel", "tensor")
gate_default_impl = "kernel"       # for GPU tensors (README "Gated graph convolution": the kernel form against the tensor form); CPU tensors take "tensor"


def _gate_impl(impl, t):
    """The form one call runs: the argument, else the BOT_GATE variable (read at call time), else the default for the tensor's device."""
    if impl is None:
        impl = os.environ.get("BOT_GATE") or (gate_default_impl if t.is_cuda else "tensor")
    if impl not in GATE_IMPLS:
        raise ValueError(f"gated_sum: impl (or BOT_GATE) must be one of {GATE_IMPLS}, got {impl!r}")
    return impl


def _unit_rows(x):
    """[n, F] as the sweeps take it: unit inner stride (the row stride may be wider: a column block of a merged projection stays a view)."""
    return x if x.shape[1] == 1 or x.stride(1) == 1 else x.contiguous()


class _GatedSum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, k, q, v, normalize, eps):
        k, q, v = _unit_rows(k), _unit_rows(q), _unit_rows(v)
        out, den = _C.spmm_gate(g.csc, k, q, v, normalize, eps)
        ctx.g, ctx.normalize, ctx.eps = g, normalize, eps
        if normalize:
            ctx.save_for_backward(k, q, v, out, den)
        else:
            ctx.save_for_backward(k, q, v)
        return out

    @staticmethod
    def backward(ctx, dout):
        g = ctx.g
        need_k, need_q, need_v = ctx.needs_input_grad[1:4]
        dk = dq = dv = None
        if not (need_k or need_q or need_v):
            return None, None, None, None, None, None
        if ctx.normalize:               # out = num / (den + eps):  d num = a,  d den = b = -a out  (dense passes over [n_dst, F])
            k, q, v, out, den = ctx.saved_tensors
            a = dout / (den + ctx.eps)
            b = -a * out
        else:
            k, q, v = ctx.saved_tensors
            a, b = dout.contiguous(), None
        if need_k:
            dk = _C.spmm_gate_bwd_dst(g.csc, k, q, v, a, b)
        if need_q or need_v:            # the CSR is built here: only when a source-side gradient is asked for
            dq, dv = _C.spmm_gate_bwd_src(g.csr, k, q, v, a, b, want_dq=need_q, want_dv=need_v)
        return None, dk, dq, dv, None, None


def gated_sum_positions(g, k, q, v, normalize=False, eps=1e-6):
    """The tensor form of `gated_sum`: gathers to [E, F] in CSC position order, a sigmoid, a product and one (normalised: two) segment
    sums in torch ops, differentiable in k, q and v; it materialises [E, F] tensors in both passes."""
    n_dst, E, F = g.number_of_dst_nodes(), g.csc.nnz, k.shape[1]
    deg = (g.csc.indptr[1:] - g.csc.indptr[:-1]).long()
    seg = torch.repeat_interleave(torch.arange(n_dst, device=k.device), deg, output_size=E)
    idx = g.csc.indices
    gate = torch.sigmoid(take_rows(k, seg) + take_rows(q, idx))
    zeros = torch.zeros((n_dst, F), dtype=k.dtype, device=k.device)
    num = zeros.index_add(0, seg, gate * take_rows(v, idx))
    if not normalize:
        return num
    den = zeros.index_add(0, seg, gate)
    return torch.where((deg > 0).reshape(-1, 1), num / (den + eps), zeros)      # an empty row: 0 whatever eps is


def gated_sum(g, k, q, v, normalize=False, eps=1e-6, impl=None):
    """The gated aggregation of Bresson & Laurent's residual gated graph ConvNets (arXiv:1711.07553; the GatedGCN of "Benchmarking Graph
    Neural Networks", PyG's ResGatedGraphConv), per destination w and column f over the in-edges u -> w:

        num[w, f] = sum_u sigmoid(k[w, f] + q[u, f]) v[u, f];   den[w, f] = sum_u sigmoid(k[w, f] + q[u, f])
        out = num,  or - normalize - num / (den + eps)          (a destination without in-edges gets 0)

    k: [n_dst, F]; q, v: [n_src, F] (on a block n_dst < n_src); q and v may be the two column blocks of one [n_src, 2F] projection, which
    the kernels then gather as one row.  impl="kernel" (float32): one sweep over the CSC, one more for dk and one over the CSR for dq and
    dv (csrc/spmm_gate.hip); the gates are formed again in the backward, nothing of size [E, F] exists, no atomics, and a gradient that is
    not needed is not computed (the CSR is built only for dq or dv).  impl="tensor": `gated_sum_positions`, which materialises [E, F]:
    what runs on CPU tensors and what the kernels are timed against.  impl=None: the BOT_GATE variable, else `gate_default_impl` on the
    GPU.  Whole graphs, Subgraphs and sampled blocks; a graph with a halo plan raises ValueError; wrong shapes, dtypes or devices DGLError."""
    from .errors import DGLError
    if g.halo is not None:
        raise ValueError("gated_sum on a partitioned graph (a halo plan) is not supported: it takes whole graphs, Subgraphs and sampled blocks")
    if float(eps) < 0 or float(eps) != float(eps) or float(eps) == float("inf"):
        raise ValueError(f"gated_sum: eps must be finite and not negative, got {eps!r}")
    n_src, n_dst = g.number_of_src_nodes(), g.number_of_dst_nodes()
    if k.dim() != 2 or k.shape[0] != n_dst or k.shape[1] < 1:
        raise DGLError(f"gated_sum: k must be [{n_dst}, F >= 1] (one row per destination node), got {tuple(k.shape)}")
    F = int(k.shape[1])
    for name, t in (("q", q), ("v", v)):
        if tuple(t.shape) != (n_src, F):
            raise DGLError(f"gated_sum: {name} must be [{n_src}, {F}] (one row per source node), got {tuple(t.shape)}")
        if t.dtype != k.dtype or t.device != k.device:
            raise DGLError(f"gated_sum: {name} must be {k.dtype} on {k.device} like k, got {t.dtype} on {t.device}")
    if not k.is_floating_point():
        raise DGLError(f"gated_sum: k, q and v must be floating point, got {k.dtype}")
    if g.csc.indptr.device != k.device:
        raise DGLError(f"gated_sum: the graph is on {g.csc.indptr.device}, k on {k.device}")
    if _gate_impl(impl, k) == "kernel":
        if k.dtype != torch.float32:
            raise DGLError(f"gated_sum: the kernel form takes float32, got {k.dtype}")
        return _GatedSum.apply(g, k, q, v, bool(normalize), float(eps))
    return gated_sum_positions(g, k, q, v, bool(normalize), float(eps))


gate_edge_default_impl = "kernel"  # `gated_edge_sum` on GPU tensors (README "GatedGCN with an edge stream"); CPU tensors take "tensor"


def _gate_edge_impl(impl, t):
    """The form one call runs: the argument, else the BOT_GATE_EDGE variable (read at call time), else the default for the tensor's device."""
    if impl is None:
        impl = os.environ.get("BOT_GATE_EDGE") or (gate_edge_default_impl if t.is_cuda else "tensor")
    if impl not in GATE_IMPLS:
        raise ValueError(f"gated_edge_sum: impl (or BOT_GATE_EDGE) must be one of {GATE_IMPLS}, got {impl!r}")
    return impl


class _GatedEdgeSum(torch.autograd.Function):
    """Two outputs, (out, e); c, e and their gradients in CSC position order.  Saves k, q, v, e (and out, den, normalised), not c: the
    backward forms the gates again from the stored e, and dc is ds itself."""

    @staticmethod
    def forward(ctx, g, k, q, v, c, normalize, eps, want_edge, keep):
        k, q, v, c = _unit_rows(k), _unit_rows(q), _unit_rows(v), _unit_rows(c)
        out, den, e = _C.spmm_gate_edge(g.csc, k, q, v, c, normalize, eps, want_e=want_edge or keep)   # keep: a backward will read e
        ctx.g, ctx.normalize, ctx.eps = g, normalize, eps
        ctx.set_materialize_grads(False)
        if normalize:
            ctx.save_for_backward(k, q, v, e, out, den)
        else:
            ctx.save_for_backward(k, q, v, e)
        return out, (e if want_edge else None)

    @staticmethod
    def backward(ctx, dout, de=None):
        g = ctx.g
        need_k, need_q, need_v, need_c = ctx.needs_input_grad[1:5]
        dk = dq = dv = ds = None
        if not (need_k or need_q or need_v or need_c) or (dout is None and de is None):
            return (None,) * 9
        k, q, v, e = ctx.saved_tensors[:4]
        if dout is None:
            dout = torch.zeros_like(k)
        if ctx.normalize:               # out = num / (den + eps):  d num = a,  d den = b = -a out  (dense passes over [n_dst, F])
            out, den = ctx.saved_tensors[4:]
            a = dout / (den + ctx.eps)
            b = -a * out
        else:
            a, b = dout.contiguous(), None
        if need_k or need_q or need_c:  # one sweep over the CSC: ds per position (dc, and the operand of dq) and dk
            ds, dk = _C.spmm_gate_edge_bwd(g.csc, v, e, a, b, None if de is None else _unit_rows(de), want_ds=need_q or need_c, want_dk=need_k)
        if need_q or need_v:            # the CSR is built here: only when a source-side gradient is asked for
            dq, dv = _C.spmm_gate_edge_bwd_src(g.csr, g.csr2csc, e, ds, a, want_dq=need_q, want_dv=need_v)
        return None, dk, dq, dv, (ds if need_c else None), None, None, None, None


def gated_edge_positions(g, k, q, v, c, normalize=True, eps=1e-6):
    """The tensor form of `gated_edge_sum` with c in CSC position order -> (out, e), e in position order: gathers to [E, F], two sums, a
    sigmoid, a product and one (normalised: two) segment sums in torch ops, differentiable in k, q, v and c."""
    n_dst, E, F = g.number_of_dst_nodes(), g.csc.nnz, k.shape[1]
    deg = (g.csc.indptr[1:] - g.csc.indptr[:-1]).long()
    seg = torch.repeat_interleave(torch.arange(n_dst, device=k.device), deg, output_size=E)
    idx = g.csc.indices
    e = (_take_rows_grad(k, seg) + _take_rows_grad(q, idx)) + c
    gate = torch.sigmoid(e)
    zeros = torch.zeros((n_dst, F), dtype=k.dtype, device=k.device)
    num = zeros.index_add(0, seg, gate * _take_rows_grad(v, idx))
    if not normalize:
        return num, e
    den = zeros.index_add(0, seg, gate)
    return torch.where((deg > 0).reshape(-1, 1), num / (den + eps), zeros), e      # an empty row: 0 whatever eps is


def _edge_rows_long(g):
    """`_csc_edge_rows` as int64 (what index ops take), cached on the graph; None where an edge's id is its position."""
    perm = _csc_edge_rows(g)
    if perm is None:
        return None
    cache = getattr(g, "_bot_cache", None)
    if cache is None:
        cache = g._bot_cache = {}
    hit = cache.get("csc_eid_long")
    if hit is None or hit[0] is not perm:
        hit = cache["csc_eid_long"] = (perm, perm.long())
    return hit[1]


def gated_edge_sum(g, k, q, v, c, normalize=True, eps=1e-6, order="eid", want_edge=True, impl=None):
    """GatedGCN's aggregation with an edge stream ("Benchmarking Graph Neural Networks", arXiv:2003.00982; GraphGPS's local layer; DGL's
    GatedGCNConv): `gated_sum` whose gate has a per-edge term and whose pre-activation is the second output.  Per edge j = u -> w:

        e[j]   = (k[w] + q[u]) + c[j]
        num[w] = sum_j sigmoid(e[j]) v[u];   den[w] = sum_j sigmoid(e[j])
        out    = num,  or - normalize - num / (den + eps)          (a destination without in-edges gets 0)

    Returns (out [n_dst, F], e [E, F]), or (out, None) with want_edge=False.  k: [n_dst, F]; q, v: [n_src, F] (they may be the two column
    blocks of one [n_src, 2F] projection); c: [E, F].  order="eid": c comes in and e goes out in edge-id order - one row permutation each
    way on a graph whose edge ids are not its CSC positions, none on a Block or Subgraph; order="csc": CSC position order on both sides,
    no permutation (what a stack keeps between its layers).  impl="kernel" (float32): one sweep over the CSC that stores e, one more for
    ds (= dc) and dk from the stored e, and one over the CSR for dq and dv (csrc/spmm_gate_edge.hip); k, q, v, e (and out, den) are
    saved, c is not; no atomics; a gradient that is not needed is not computed, the CSR is built only for dq or dv, and with
    want_edge=False under no_grad nothing per edge is written.  impl="tensor": `gated_edge_positions`, which materialises the gathers,
    the sigmoid and the product as [E, F] tensors: what runs on CPU tensors and what the kernels are timed against.  impl=None: the
    BOT_GATE_EDGE variable, else `gate_edge_default_impl` on the GPU.  Whole graphs, Subgraphs and sampled blocks; a graph with a halo
    plan raises ValueError; wrong shapes, dtypes or devices DGLError."""
    from .errors import DGLError
    if g.halo is not None:
        raise ValueError("gated_edge_sum on a partitioned graph (a halo plan) is not supported: it takes whole graphs, Subgraphs and sampled blocks")
    if float(eps) < 0 or float(eps) != float(eps) or float(eps) == float("inf"):
        raise ValueError(f"gated_edge_sum: eps must be finite and not negative, got {eps!r}")
    if order not in ("eid", "csc"):
        raise ValueError(f'gated_edge_sum: order must be "eid" or "csc", got {order!r}')
    n_src, n_dst, E = g.number_of_src_nodes(), g.number_of_dst_nodes(), g.csc.nnz
    if k.dim() != 2 or k.shape[0] != n_dst or k.shape[1] < 1:
        raise DGLError(f"gated_edge_sum: k must be [{n_dst}, F >= 1] (one row per destination node), got {tuple(k.shape)}")
    F = int(k.shape[1])
    for name, t, n, what in (("q", q, n_src, "source node"), ("v", v, n_src, "source node"), ("c", c, E, "edge")):
        if tuple(t.shape) != (n, F):
            raise DGLError(f"gated_edge_sum: {name} must be [{n}, {F}] (one row per {what}), got {tuple(t.shape)}")
        if t.dtype != k.dtype or t.device != k.device:
            raise DGLError(f"gated_edge_sum: {name} must be {k.dtype} on {k.device} like k, got {t.dtype} on {t.device}")
    if not k.is_floating_point():
        raise DGLError(f"gated_edge_sum: k, q, v and c must be floating point, got {k.dtype}")
    if g.csc.indptr.device != k.device:
        raise DGLError(f"gated_edge_sum: the graph is on {g.csc.indptr.device}, k on {k.device}")
    kernel = _gate_edge_impl(impl, k) == "kernel"
    if kernel and k.dtype != torch.float32:
        raise DGLError(f"gated_edge_sum: the kernel form takes float32, got {k.dtype}")
    perm = _edge_rows_long(g) if order == "eid" else None
    if perm is not None:
        c = _take_rows_grad(c, perm)
    if kernel:
        keep = torch.is_grad_enabled() and any(t.requires_grad for t in (k, q, v, c))     # (forward itself runs with gradients off)
        out, e = _GatedEdgeSum.apply(g, k, q, v, c, bool(normalize), float(eps), bool(want_edge), keep)
    else:
        out, e = gated_edge_positions(g, k, q, v, c, bool(normalize), float(eps))
    if not want_edge:
        return out, None
    if perm is not None:
        e = torch.empty_like(e).index_copy(0, perm, e)
    return out, e


REL_IMPLS = ("kernel", "tensor")
rel_default_impl = "kernel"       # for GPU tensors (README "R-GCN": the kernel form against the tensor and loop forms); CPU tensors take "tensor"


def _rel_impl(impl, t, who):
    """The form one call runs: the argument, else the BOT_REL variable (read at call time), else the default for the tensor's device."""
    if impl is None:
        impl = os.environ.get("BOT_REL") or (rel_default_impl if t.is_cuda else "tensor")
    if impl not in REL_IMPLS:
        raise ValueError(f"{who}: impl (or BOT_REL) must be one of {REL_IMPLS}, got {impl!r}")
    return impl


def _rel_cached(g, t, tag, make):
    """`make()` once per graph and per (tensor identity, version) of the constant per-edge tensor `t`, as `edge_features_csc` keeps its
    copy.  Whenever an entry is made, the entries of tensors that are gone and of earlier versions of `t` leave (with what hung on them:
    the int32 copy of a freed `etypes` takes its position copies and its relation direction along), so relations or norms that are
    rewritten every epoch do not pile up on a long-lived graph."""
    cache = getattr(g, "_bot_cache", None)
    if cache is None:
        cache = g._bot_cache = {}
    key = ("rel", tag, t.data_ptr(), t._version, tuple(t.shape), t.dtype)
    hit = cache.get(key)
    if hit is None or hit[0]() is not t:            # (an address is reused once its tensor is freed: the entry must be this very tensor's)
        made = make()
        stale = True
        while stale:                                # dropping an entry may free the tensor that others are keyed on
            stale = [k for k, v in cache.items() if isinstance(k, tuple) and k[0] == "rel" and
                     (v[0]() is None or (v[0]() is t and k[3] != t._version))]
            for k in stale:
                del cache[k]
        hit = cache[key] = (weakref.ref(t), made)
    return hit[1]


def _rel_positions(g, t, which):
    """The per-edge constant `t` ([E] in edge-id order: the relations as int32, or the norm) in the position order of g.csc / g.csr."""
    d = g.csc if which == "csc" else g.csr
    return _rel_cached(g, t, "rel_" + which, lambda: take_rows(t, d.eid).contiguous())


def _rel_direction(g, et, num_rels):
    """The "relation direction" of the int32 relations `et`: `build_direction` with the relations as rows over the CSC POSITIONS, so a
    segment sum per relation folds a relation's million edges as long-row chunks in slot order.  Cached beside the position copies."""
    from .graph import build_direction

    def make():
        rows = _rel_positions(g, et, "csc").long()
        return build_direction(rows, torch.arange(rows.numel(), device=rows.device), num_rels)
    return _rel_cached(g, et, "rel_dir", make)


def _rel_dcoef(g, dots, et, nm, shape):
    """dcoef [R, B] from the per-position dots [E, B] (CSC position order): times the norm, then the segment sum over the relation
    direction - no float atomics, nothing of size [E, F]."""
    if nm is not None:
        dots = dots * _rel_positions(g, nm, "csc").unsqueeze(1)
    d = _rel_direction(g, et, shape[0])
    return _C.segment_sum(d, dots, d.eid).view(shape)


class _RelExpand(torch.autograd.Function):
    """Z = expand(x) over the CSC; dx = contract(dZ) over the CSR with the same coefficients; dcoef from per-position dots."""

    @staticmethod
    def forward(ctx, g, x, coef, et, nm, num_rels):
        x = _unit_rows(x)
        coef = None if coef is None else coef.contiguous()
        Z = _C.spmm_rel_expand(g.csc, x, _rel_positions(g, et, "csc"), num_rels, coef, None if nm is None else _rel_positions(g, nm, "csc"))
        ctx.g, ctx.et, ctx.nm, ctx.num_rels = g, et, nm, num_rels
        need_x, need_c = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        ctx.save_for_backward(x if need_c else None, coef if need_x else None)      # (coef None: one-hot, nothing to save)
        return Z

    @staticmethod
    def backward(ctx, dZ):
        g, et, nm = ctx.g, ctx.et, ctx.nm
        x, coef = ctx.saved_tensors
        dZ = dZ.contiguous()
        dx = dcoef = None
        if ctx.needs_input_grad[1]:             # the CSR is built here: only when the source-side gradient is asked for
            dx = _C.spmm_rel_contract(g.csr, dZ, _rel_positions(g, et, "csr"), ctx.num_rels, coef,
                                      None if nm is None else _rel_positions(g, nm, "csr"))
        if ctx.needs_input_grad[2]:
            dcoef = _rel_dcoef(g, _C.sddmm_dot_blocks(g.csc, x, dZ), et, nm, (ctx.num_rels, dZ.shape[1]))
        return None, dx, dcoef, None, None, None


class _RelContract(torch.autograd.Function):
    """out = contract(y) over the CSC; dy = expand(dout) over the CSR with the same coefficients; dcoef from per-position dots."""

    @staticmethod
    def forward(ctx, g, y, coef, et, nm, num_rels):
        y = y.contiguous() if (y.stride(2) != 1 and y.shape[2] > 1) or (y.shape[1] > 1 and y.stride(1) != y.shape[2]) else y
        coef = None if coef is None else coef.contiguous()
        out = _C.spmm_rel_contract(g.csc, y, _rel_positions(g, et, "csc"), num_rels, coef, None if nm is None else _rel_positions(g, nm, "csc"))
        ctx.g, ctx.et, ctx.nm, ctx.num_rels = g, et, nm, num_rels
        need_y, need_c = ctx.needs_input_grad[1], ctx.needs_input_grad[2]
        ctx.save_for_backward(y if need_c else None, coef if need_y else None)
        return out

    @staticmethod
    def backward(ctx, dout):
        g, et, nm = ctx.g, ctx.et, ctx.nm
        y, coef = ctx.saved_tensors
        dout = _unit_rows(dout)
        dy = dcoef = None
        if ctx.needs_input_grad[1]:             # the CSR is built here: only when the source-side gradient is asked for
            dy = _C.spmm_rel_expand(g.csr, dout, _rel_positions(g, et, "csr"), ctx.num_rels, coef,
                                    None if nm is None else _rel_positions(g, nm, "csr"))
        if ctx.needs_input_grad[2]:             # <y[u, b], dout[v]>: the B blocks as heads, dout repeated per block ([n_dst, B, F], not [E, F])
            B = y.shape[1]
            dots = _C.sddmm_dot(g.csc, y, dout.unsqueeze(1).expand(dout.shape[0], B, dout.shape[1]).contiguous())
            dcoef = _rel_dcoef(g, dots, et, nm, (ctx.num_rels, B))
        return None, dy, dcoef, None, None, None


def _rel_weights(g, et, nm, num_rels, coef, dtype):
    """Tensor form: the weight row c_e coef[r_e, :] of every CSC position -> [E, B] (one-hot: None, the norm [E, 1] or None apart)."""
    c = None if nm is None else _rel_positions(g, nm, "csc").to(dtype).unsqueeze(1)
    if coef is None:
        return None, c
    w = coef[_rel_positions(g, et, "csc").long()]
    return (w if c is None else w * c), c


def rel_expand_positions(g, x, et, nm, num_rels, coef=None):
    """The tensor form of `rel_expand_sum`: per coefficient column one [E, F] message tensor and one `index_add` (one-hot: one of each
    into the [n_dst * R, F] view), differentiable in x and coef."""
    n_dst, F = g.number_of_dst_nodes(), x.shape[1]
    seg, xg = csc_destinations(g), take_rows(x, g.csc.indices)
    w, c = _rel_weights(g, et, nm, num_rels, coef, x.dtype)
    if coef is None:
        rows = seg * num_rels + _rel_positions(g, et, "csc").long()
        Z = torch.zeros((n_dst * num_rels, F), dtype=x.dtype, device=x.device).index_add(0, rows, xg if c is None else xg * c)
        return Z.view(n_dst, num_rels, F)
    zeros = torch.zeros((n_dst, F), dtype=x.dtype, device=x.device)
    return torch.stack([zeros.index_add(0, seg, w[:, b:b + 1] * xg) for b in range(coef.shape[1])], dim=1)


def rel_contract_positions(g, y, et, nm, num_rels, coef=None):
    """The tensor form of `rel_contract_sum`: the [E, F] message sum_b c_e coef[r_e, b] y[u_e, b] (one-hot: c_e y[u_e, r_e]) and one
    `index_add`, differentiable in y and coef."""
    n_dst, B, F = g.number_of_dst_nodes(), y.shape[1], y.shape[2]
    seg, idx = csc_destinations(g), g.csc.indices.long()
    w, c = _rel_weights(g, et, nm, num_rels, coef, y.dtype)
    if coef is None:
        m = take_rows(y.reshape(-1, F), idx * num_rels + _rel_positions(g, et, "csc").long())
        m = m if c is None else m * c
    else:
        m = sum(w[:, b:b + 1] * take_rows(y[:, b], idx) for b in range(B))
    return torch.zeros((n_dst, F), dtype=y.dtype, device=y.device).index_add(0, seg, m)


def _rel_prologue(who, g, t, etypes, num_rels, coef, norm, impl):
    """What `rel_expand_sum` and `rel_contract_sum` check and set up -> (relations int32 [E], norm [E] or None, impl).  The relations'
    range is read once per graph and tensor (one host read of min and max), when their cache entry is made."""
    from .errors import DGLError
    if g.halo is not None:
        raise ValueError(f"{who} on a partitioned graph (a halo plan) is not supported: it takes whole graphs, Subgraphs and sampled blocks")
    E = g.number_of_edges()
    if isinstance(num_rels, bool) or not isinstance(num_rels, int) or num_rels < 1:
        raise DGLError(f"{who}: num_rels must be an integer >= 1, got {num_rels!r}")
    if not isinstance(t, torch.Tensor) or not t.is_floating_point():
        raise DGLError(f"{who}: the features must be a floating point tensor, got {getattr(t, 'dtype', type(t).__name__)}")
    if isinstance(etypes, str):
        if etypes not in g.edata:
            raise DGLError(f"{who}: the graph has no edata[{etypes!r}]")
        etypes = g.edata[etypes]
    if not isinstance(etypes, torch.Tensor) or etypes.dtype not in (torch.int32, torch.int64) or tuple(etypes.shape) != (E,):
        raise DGLError(f"{who}: etypes must be an int32 or int64 tensor [{E}] (one relation per edge, edge-id order) or an edata key, got "
                       f"{tuple(etypes.shape) if isinstance(etypes, torch.Tensor) else type(etypes).__name__} "
                       f"{getattr(etypes, 'dtype', '')}")
    if isinstance(norm, str):
        if norm not in g.edata:
            raise DGLError(f"{who}: the graph has no edata[{norm!r}]")
        norm = g.edata[norm]
    if norm is not None:
        if not isinstance(norm, torch.Tensor) or norm.dtype != torch.float32 or tuple(norm.shape) not in ((E,), (E, 1)):
            raise DGLError(f"{who}: norm must be a float32 tensor [{E}] or [{E}, 1] (edge-id order) or an edata key, got "
                           f"{tuple(norm.shape) if isinstance(norm, torch.Tensor) else type(norm).__name__} {getattr(norm, 'dtype', '')}")
    if coef is not None:
        if not isinstance(coef, torch.Tensor) or coef.dim() != 2 or coef.shape[0] != num_rels or coef.shape[1] < 1:
            raise DGLError(f"{who}: coef must be [num_rels = {num_rels}, B >= 1], got {tuple(getattr(coef, 'shape', ()))}")
        if coef.dtype != t.dtype:
            raise DGLError(f"{who}: coef must be {t.dtype} like the features, got {coef.dtype}")
    for name, o in (("etypes", etypes), ("norm", norm), ("coef", coef), ("the graph", g.csc.indptr)):
        if o is not None and o.device != t.device:
            raise DGLError(f"{who}: {name} is on {o.device}, the features on {t.device}")
    impl = _rel_impl(impl, t, who)
    if impl == "kernel" and t.dtype != torch.float32:
        raise DGLError(f"{who}: the kernel form takes float32, got {t.dtype}")

    def check_range():
        if E:
            lo, hi = torch.stack((etypes.min(), etypes.max())).tolist()         # one host read
            if lo < 0 or hi >= num_rels:
                raise DGLError(f"{who}: etypes must lie in [0, num_rels = {num_rels}), found {lo} .. {hi}")
        return etypes.to(torch.int32, copy=True).contiguous()         # the cache's own copy: an entry must not keep the caller's tensor alive
    et = _rel_cached(g, etypes, ("rel_et", num_rels), check_range)
    nm = None if norm is None else _rel_cached(g, norm, "rel_nm", lambda: norm.detach().reshape(E).clone(memory_format=torch.contiguous_format))  # likewise
    return et, nm, impl


def rel_expand_sum(g, x, etypes, num_rels, coef=None, norm=None, impl=None):
    """The expand sweep of the relational GCN (Schlichtkrull et al., ESWC 2018; DGL's RelGraphConv, PyG's RGCNConv) with the basis
    regulariser W_r = sum_b coef[r, b] V_b, over the in-edges e = (u -> v) with relation r_e and constant weight c_e:

        Z[v, b, :] = sum_e c_e coef[r_e, b] x[u, :]          x [n_src, F] -> Z [n_dst, B, F]

    so that `Z.view(n_dst, B * F) @ V.view(B * F, F_out)` is the layer's relation part (aggregate-first).  coef [num_rels, B], or None:
    the one-hot mode, B = num_rels and coef the identity (never stored; a row is added into block r_e alone).  etypes: int32 / int64 [E]
    in edge-id order, or an edata key; their range is checked once per graph (DGLError).  norm: float32 [E] or [E, 1] (edge-id order) or
    an edata key; it is a constant and gets no gradient.  impl="kernel" (float32): one sweep over the CSC (csrc/spmm_rel.hip), B <= 16
    accumulator blocks per pass; the gradient of x is the contract sweep over the CSR (built only when that gradient is needed), the
    gradient of coef per-position dots [E, B] and a segment sum per relation; no atomics, nothing of size [E, F].  impl="tensor": the
    same contract in torch ops (what CPU tensors run).  impl=None: the BOT_REL variable, else `rel_default_impl` on the GPU.  Whole
    graphs, Subgraphs and sampled blocks; a halo plan raises ValueError, wrong shapes, dtypes or devices DGLError."""
    from .errors import DGLError
    et, nm, impl = _rel_prologue("rel_expand_sum", g, x, etypes, num_rels, coef, norm, impl)
    if x.dim() != 2 or x.shape[0] != g.number_of_src_nodes() or x.shape[1] < 1:
        raise DGLError(f"rel_expand_sum: x must be [{g.number_of_src_nodes()}, F >= 1] (one row per source node), got {tuple(x.shape)}")
    if impl == "kernel":
        return _RelExpand.apply(g, x, coef, et, nm, num_rels)
    return rel_expand_positions(g, x, et, nm, num_rels, coef)


def rel_contract_sum(g, y, etypes, num_rels, coef=None, norm=None, impl=None):
    """The contract sweep, `rel_expand_sum`'s transpose (same arguments), for the project-first order y = x @ [V_1 | ... | V_B]:

        out[v, :] = sum_e c_e sum_b coef[r_e, b] y[u, b, :]     y [n_src, B, F] -> out [n_dst, F]

    With coef=None (one-hot, y [n_src, num_rels, F]) only block r_e of the source row is gathered.  The gradient of y is the expand
    sweep over the CSR."""
    from .errors import DGLError
    et, nm, impl = _rel_prologue("rel_contract_sum", g, y, etypes, num_rels, coef, norm, impl)
    B = num_rels if coef is None else coef.shape[1]
    if y.dim() != 3 or y.shape[0] != g.number_of_src_nodes() or y.shape[1] != B or y.shape[2] < 1:
        raise DGLError(f"rel_contract_sum: y must be [{g.number_of_src_nodes()}, {B}, F >= 1] (one row per source node, one block per "
                       f"{'relation' if coef is None else 'basis'}), got {tuple(y.shape)}")
    if impl == "kernel":
        return _RelContract.apply(g, y, coef, et, nm, num_rels)
    return rel_contract_positions(g, y, et, nm, num_rels, coef)


DOT_ATTN_IMPLS = ("kernel", "tensor")
dot_attn_default_impl = "kernel"   # for GPU tensors (README "Dot-product attention": the kernel form against the tensor form); CPU tensors take "tensor"
dot_attn_last_impl = None          # the form the last call of dot_attention ran
DOT_ATTN_MAX_HEAD_LANES = 64 * 6   # csrc/dot_attn.hip: one head must fit a tile of 64 lanes x 6 chunks of 4 / 2 / 1 floats


def _dot_attn_impl(impl, t):
    """The form one call asks for: the argument, else the BOT_DOT_ATTN variable (read at call time), else the default for the device."""
    if impl is None:
        impl = os.environ.get("BOT_DOT_ATTN") or (dot_attn_default_impl if t.is_cuda else "tensor")
    if impl not in DOT_ATTN_IMPLS:
        raise ValueError(f"dot_attention: impl (or BOT_DOT_ATTN) must be one of {DOT_ATTN_IMPLS}, got {impl!r}")
    return impl


def dot_attn_head_fits(D, *rows):
    """Whether a head of D columns fits one tile of the sweeps (csrc/dot_attn.hip) for operands `rows` ([n, H, D] with contiguous rows):
    D / vec <= 384 with vec the largest of 4 / 2 / 1 that divides D and keeps every row aligned (common.h pick_vec)."""
    vec = 1
    for w in (4, 2):
        if D % w == 0 and all((t.shape[0] <= 1 or t.stride(0) % w == 0) and t.data_ptr() % (4 * w) == 0 for t in rows):
            vec = w
            break
    return D // vec <= DOT_ATTN_MAX_HEAD_LANES


def pack_keep(keep):
    """A bool [E, H <= 32] keep mask -> the int32 [E] words the sweeps read: bit h = head h of that position is kept."""
    H = keep.shape[1]
    bits = (keep.to(torch.int64) << torch.arange(H, device=keep.device)).sum(1)
    return torch.where(bits >= 2 ** 31, bits - 2 ** 32, bits).to(torch.int32).contiguous()


def _dot_attn_dout(dout):
    """The incoming gradient as the sweeps read it: contiguous, and 16-byte aligned - a view at an odd storage offset would narrow the
    sweeps' vectors, and with them the widest head that fits, below what the forward ran with."""
    d = dout.contiguous()
    return d.clone() if d.data_ptr() % 16 else d


def _dot_attn_bwd_src(g, q, d, pw, ds, scale, need_k, need_v, shared=False):
    """(dk, dv) from the stored p and ds - the edge term reaches them only through those, so both Functions run the one sweep over the
    sources.  The CSR is built here: only when k or v needs a gradient."""
    if not (need_k or need_v):
        return None, None
    if shared:                              # one tensor came in twice: its gradient is dk + dv, handed back once
        return _C.dot_attn_bwd_src(g.csr, g.csr2csc, q, d, pw, ds, scale, shared=True)[0], None
    return _C.dot_attn_bwd_src(g.csr, g.csr2csc, q, d, pw, ds, scale, want_dk=need_k, want_dv=need_v)


class _DotAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, q, k, v, scale, keep, p, shared):
        v = k if shared else v                   # (rows already contiguous: dot_attention)
        out, lse = _C.dot_attn(g.csc, q, k, v, scale, keep, p)
        ctx.g, ctx.scale, ctx.p, ctx.shared, ctx.keep = g, scale, p, shared, keep
        ctx.save_for_backward(q, k, v, out, lse)
        return out

    @staticmethod
    def backward(ctx, dout):
        g = ctx.g
        q, k, v, out, lse = ctx.saved_tensors
        _, need_q, need_k, need_v = ctx.needs_input_grad[:4]
        d = _dot_attn_dout(dout)
        dq, pw, ds = _C.dot_attn_bwd_dst(g.csc, q, k, v, ctx.scale, ctx.keep, ctx.p, d, out, lse, want_dq=need_q)
        dk, dv = _dot_attn_bwd_src(g, q, d, pw, ds, ctx.scale, need_k, need_v, ctx.shared)
        return None, dq, dk, dv, None, None, None, None


def csc_destinations(g):
    """The destination of every CSC position: int64 [E]."""
    deg = (g.csc.indptr[1:] - g.csc.indptr[:-1]).long()
    return torch.repeat_interleave(torch.arange(g.number_of_dst_nodes(), device=deg.device), deg, output_size=g.csc.indices.numel())


def _dot_attn_prologue(name, g, q, k, v, scale, keep, p, impl, ef=None, weight=None):
    """What `dot_attention` and `dot_attention_edge` (ef, weight given) check and set up, under the op's `name` -> (H, D, E, scale, keep,
    p, impl): the operands' shapes, the p range, the mask (drawn when p > 0 comes without one; p = 0 without a mask), the scale's
    default and the form asked for."""
    if g.halo is not None:
        raise ValueError(f"{name} on a partitioned graph (a halo plan) is not supported: it takes whole graphs, Subgraphs and sampled blocks")
    if q.dim() != 3 or q.shape[0] != g.number_of_dst_nodes():
        raise ValueError(f"{name}: q must be [{g.number_of_dst_nodes()}, H, D] (one row per destination node), got {tuple(q.shape)}")
    H, D = int(q.shape[1]), int(q.shape[2])
    n_src, E = g.number_of_src_nodes(), g.number_of_edges()
    for what, t in (("k", k), ("v", v)):
        if tuple(t.shape) != (n_src, H, D):
            raise ValueError(f"{name}: {what} must be [{n_src}, {H}, {D}] (one row per source node), got {tuple(t.shape)}")
    if H < 1 or D < 1:
        raise ValueError(f"{name}: H and D must be at least 1, got q {tuple(q.shape)}")
    if ef is not None:
        if ef.dim() != 2 or ef.shape[0] != E or ef.shape[1] < 1:
            raise ValueError(f"{name}: ef must be [{E}, K >= 1] (one row per edge, edge-id order), got {tuple(ef.shape)}")
        K = int(ef.shape[1])
        if tuple(weight.shape) != (H * D, K):
            raise ValueError(f"{name}: weight must be [{H * D}, {K}] (as nn.Linear({K}, {H * D}, bias=False) stores it), got "
                             f"{tuple(weight.shape)}")
        for what, t in (("k", k), ("v", v), ("ef", ef), ("weight", weight)):
            if t.dtype != q.dtype or t.device != q.device:
                raise ValueError(f"{name}: {what} must be {q.dtype} on {q.device} like q, got {t.dtype} on {t.device}")
    p = float(p)
    if not 0.0 <= p < 1.0:
        raise ValueError(f"{name}: p must be in [0, 1), got {p}")
    if keep is not None and (tuple(keep.shape) != (E, H) or keep.dtype != torch.bool):
        raise ValueError(f"{name}: keep must be bool [{E}, {H}] in CSC position order, got {keep.dtype} {tuple(keep.shape)}")
    scale = float(D) ** -0.5 if scale is None else float(scale)
    if keep is None and p > 0.0:
        keep = torch.rand((E, H), device=q.device) >= p
    if keep is None:
        p = 0.0
    return H, D, E, scale, keep, p, _dot_attn_impl(impl, q)


def dot_attention(g, q, k, v, scale=None, *, keep=None, p=0.0, impl=None, return_attention=False):
    """Scaled dot-product attention over every destination's in-edges (the layer of UniMP, Shi et al., arXiv:2009.03509; PyG's
    TransformerConv, DGL's DotGatConv):

        a_uv = softmax over the in-edges u -> v of (q[v] . k[u] * scale)  per head;   out[v] = sum_u dropout(a_uv) v[u]

    q: float32 [n_dst, H, D]; k, v: float32 [n_src, H, D] (on a block n_dst < n_src); scale=None: D ** -0.5.  Returns [n_dst, H, D];
    a destination without in-edges gets 0.  Attention dropout: `p` with a drawn `keep` mask (bool [E, H], CSC position order) scales the
    kept weights by 1 / (1 - p); p > 0 without a mask draws one with torch's generator (`torch.rand(E, H) >= p`).
    impl="kernel": ONE sweep per forward that forms logits, online softmax and aggregation from one gather, and one sweep per direction
    for the gradients (csrc/dot_attn.hip; the CSR is built only when k or v needs a gradient; `k is v` gathers once); nothing of size
    [E, H, D] exists and the forward stores nothing per edge.  impl="tensor": `(k[src] * q[dst]).sum(-1) * scale` -> `gat_attention(ee=)`
    -> dropout -> `u_mul_e_sum`: what runs on CPU tensors, for heads too wide for the sweep's tile (D / vec > 384), for more than 32
    heads with a mask, with return_attention (-> (out, a [E, H, 1] in CSC position order, before dropout)), and what the kernels are
    timed against.  impl=None: the BOT_DOT_ATTN variable, else `dot_attn_default_impl` on the GPU.  `dot_attn_last_impl` names the form
    that ran.  A graph with a halo plan raises ValueError."""
    global dot_attn_last_impl
    H, D, E, scale, keep, p, want = _dot_attn_prologue("dot_attention", g, q, k, v, scale, keep, p, impl)
    shared = k is v
    if want == "kernel" and not return_attention and (keep is None or H <= 32):
        qc, kc = _rows_contiguous(q), _rows_contiguous(k)
        vc = kc if shared else _rows_contiguous(v)
        if not q.is_cuda or dot_attn_head_fits(D, qc, kc, vc):
            dot_attn_last_impl = "kernel"
            return _DotAttention.apply(g, qc, kc, vc, scale, None if keep is None else pack_keep(keep), p, shared)
    dot_attn_last_impl = "tensor"
    e = (take_rows(k, g.csc.indices) * take_rows(q, csc_destinations(g))).sum(-1, keepdim=True) * scale        # [E, H, 1], CSC position order
    a = gat_attention(g, None, None, e, negative_slope=1.0, order="csc", ee_order="csc")                      # the edge softmax of e
    w = a if keep is None else a * (keep.to(a.dtype) * (1.0 / (1.0 - p))).unsqueeze(-1)
    out = u_mul_e_sum(g, v, w, order="csc")
    return (out, a) if return_attention else out


class _DotAttentionEdge(torch.autograd.Function):
    """The two EDGE sweeps of csrc/dot_attn.hip around given qe = q W and position-ordered ef: -> (out, aef).  dq, dqe, dk, dv go back
    to autograd, which forms dW and the rest of dq from the two dense products around this node."""

    @staticmethod
    def forward(ctx, g, q, k, v, qe, ef, scale, keep, p):
        out, lse, aef = _C.dot_attn_edge(g.csc, q, k, v, qe, ef, scale, keep, p)
        ctx.g, ctx.scale, ctx.p, ctx.keep = g, scale, p, keep
        ctx.save_for_backward(q, k, v, qe, ef, out, lse, aef)
        return out, aef

    @staticmethod
    def backward(ctx, dout, daef):
        g = ctx.g
        q, k, v, qe, ef, out, lse, aef = ctx.saved_tensors
        _, need_q, need_k, need_v, need_qe = ctx.needs_input_grad[:5]
        d = _dot_attn_dout(dout)
        dq, dqe, pw, ds = _C.dot_attn_edge_bwd_dst(g.csc, q, k, v, qe, ef, ctx.scale, ctx.keep, ctx.p, d, daef.contiguous(), out, lse, aef,
                                                   want_dq=need_q, want_dqe=need_qe)
        dk, dv = _dot_attn_bwd_src(g, q, d, pw, ds, ctx.scale, need_k, need_v)
        return None, dq, dk, dv, dqe, None, None, None, None


DOT_ATTN_EDGE_MAX_K = _C.DOT_EDGE_MAX_K      # csrc/dot_attn.hip: the widest raw edge feature of the kernel form


def dot_attention_edge(g, q, k, v, ef, weight, scale=None, *, keep=None, p=0.0, impl=None, return_attention=False):
    """`dot_attention` with K raw edge features projected into the key and the value (PyG's `TransformerConv(edge_dim=K)`; UniMP on
    graphs with edge features): with E_e = (weight @ ef[e]).view(H, D) for the edge e = u -> v,

        a_e = softmax over the in-edges of v of (q[v] . (k[u] + E_e) * scale)  per head;   out[v] = sum_e dropout(a_e) (v[u] + E_e)

    q: float32 [n_dst, H, D]; k, v: float32 [n_src, H, D]; ef: [E, K] RAW, in EDGE-ID order (on a Block or Subgraph that is the CSC
    position); weight: [H * D, K], as `nn.Linear(K, H * D, bias=False)` stores it; scale, keep, p as `dot_attention`.  Returns
    [n_dst, H, D].  Gradients: q, k, v, weight; `ef` gets one only from the tensor form.
    impl="kernel": both uses of E_e are linear, so the encoder stays outside the sweep.  qe = einsum(q, W) ([n_dst, H, K], W = weight
    viewed [H, D, K]) is a dense product in front of ONE forward sweep that reads an edge's K raw floats beside its k and v rows and
    also reduces aef = sum_e dropout(a_e) ef[e] ([n_dst, H, K]); the result is out + einsum(aef, W).  One sweep over the CSC for dq and
    dqe and `dot_attention`'s sweep over the CSR for dk and dv; dweight is autograd's, through the two dense products
    (csrc/dot_attn.hip, the EDGE instances).  Nothing of size [E, H, D] exists.  impl="tensor": `E = (ef_pos @ weight.T).view(E, H, D)`, logits
    `((k[src] + E) * q[dst]).sum(-1) * scale` -> `gat_attention(ee=)` -> dropout -> the segment sum of `a * (v[src] + E)`: what runs on
    CPU tensors, with return_attention (-> (out, a [E, H, 1] in CSC position order, before dropout)), when `ef` requires a gradient,
    for K > 16, D < K, heads too wide for the sweep's tile and more than 32 heads with a mask, and what the kernels are timed
    against.  impl=None: the BOT_DOT_ATTN variable, else `dot_attn_default_impl` on the GPU.  `dot_attn_last_impl` names the form that
    ran.  A graph with a halo plan raises ValueError, and so does the tensor form when a gradient is asked for on more than 2^24 edges
    (`graph.take_rows` gathers those in pieces, which carry no gradient)."""
    global dot_attn_last_impl
    H, D, E, scale, keep, p, want = _dot_attn_prologue("dot_attention_edge", g, q, k, v, scale, keep, p, impl, ef, weight)
    K = int(ef.shape[1])
    rows = _csc_edge_rows(g)
    ef_grad = ef.requires_grad and torch.is_grad_enabled()
    W = weight.view(H, D, K)
    if (want == "kernel" and not return_attention and not ef_grad and K <= DOT_ATTN_EDGE_MAX_K and D >= K and (keep is None or H <= 32)):
        qc, kc, vc = _rows_contiguous(q), _rows_contiguous(k), _rows_contiguous(v)
        if not q.is_cuda or dot_attn_head_fits(D, qc, kc, vc):
            dot_attn_last_impl = "kernel"
            ef_pos = ef.contiguous() if rows is None else edge_features_csc(g, ef)
            qe = torch.einsum("nhd,hdk->nhk", q, W).contiguous()      # (the product comes back head-major)
            out, aef = _DotAttentionEdge.apply(g, qc, kc, vc, qe, ef_pos, scale, None if keep is None else pack_keep(keep), p)
            return out + torch.einsum("nhk,hdk->nhd", aef, W)
    dot_attn_last_impl = "tensor"
    if E > _TAKE_CHUNK and torch.is_grad_enabled() and any(t.requires_grad for t in (q, k, v, ef, weight)):
        raise ValueError(f"dot_attention_edge: the tensor form has no gradient on a graph of {E} edges: beyond {_TAKE_CHUNK} "
                         "positions `graph.take_rows` gathers in pieces, which carry none.  The kernel form has no such limit (it needs "
                         "K <= 16, D >= K, at most 32 heads with a mask and an `ef` that requires no gradient)")
    ee = ((ef if rows is None else take_rows(ef, rows)) @ weight.t()).view(E, H, D)                              # [E, H, D], CSC position order
    e = ((take_rows(k, g.csc.indices) + ee) * take_rows(q, csc_destinations(g))).sum(-1, keepdim=True) * scale
    a = gat_attention(g, None, None, e, negative_slope=1.0, order="csc", ee_order="csc")                      # the edge softmax of e
    w = a if keep is None else a * (keep.to(a.dtype) * (1.0 / (1.0 - p))).unsqueeze(-1)
    out = _segment_sum_positions(g, w * (take_rows(v, g.csc.indices) + ee))
    return (out, a) if return_attention else out


class _SegmentSumPositions(torch.autograd.Function):
    """The sum of position-ordered per-edge rows over every destination's positions; the gradient is the destination's row per position."""

    @staticmethod
    def forward(ctx, g, m):
        ctx.g, ctx.shape = g, m.shape
        return _C.segment_sum(g.csc, _flat2(m).contiguous(), None).view((g.number_of_dst_nodes(),) + tuple(m.shape[1:]))

    @staticmethod
    def backward(ctx, dout):
        return None, take_rows(_flat2(dout), csc_destinations(ctx.g)).view(ctx.shape)


def _segment_sum_positions(g, m):
    return _SegmentSumPositions.apply(g, m)


class _UMulESum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, x, a, order, addend=None):
        x3, a2 = _as3(x), _edge2(a)
        ctx.g, ctx.order, ctx.xshape, ctx.ashape = g, order, x.shape, a.shape
        ctx.save_for_backward(x3, a2)
        wperm = g.csc.eid if order == "eid" else None
        ad3 = None if addend is None else _as3(addend)
        return _C.spmm(g.csc, x3, a2, wperm, addend=ad3).view((g.number_of_dst_nodes(),) + tuple(x.shape[1:]))

    @staticmethod
    def backward(ctx, dout):
        g = ctx.g
        x3, a2 = ctx.saved_tensors
        d3 = _as3(dout.contiguous())
        dx = da = None
        if ctx.needs_input_grad[1] and ctx.needs_input_grad[2] and x3.shape[2] <= _C.spmm_dot_max_d(d3):
            # one sweep over the out-edges yields both gradients: each gathered dout row is used twice
            wperm = g.csr.eid if ctx.order == "eid" else g.csr2csc
            dx, da = _C.spmm_dot(g.csr, d3, a2, wperm, x3)
            return None, dx.view(ctx.xshape), da.view(ctx.ashape), None, (dout if ctx.needs_input_grad[4] else None)
        if ctx.needs_input_grad[1]:
            wperm = g.csr.eid if ctx.order == "eid" else g.csr2csc
            dx = _C.spmm(g.csr, d3, a2, wperm).view(ctx.xshape)
        if ctx.needs_input_grad[2]:
            operm = g.csc.eid if ctx.order == "eid" else None
            da = _C.sddmm_dot(g.csc, x3, d3, operm).view(ctx.ashape)
        return None, dx, da, None, (dout if ctx.needs_input_grad[4] else None)


def u_mul_e_sum(g, x, a, order="eid", addend=None):
    """`update_all(fn.u_mul_e('ft','a','m'), fn.sum('m','ft'))` — models.py:547.
    x: [N,H,D]; a: [E,H,1] (or [E,H]) in edge-id order, or in CSC position order with order="csc".
    `addend` [N_dst,H,D]: added to the result in the kernel's epilogue (`rst + dst_fc(feat_dst)`, ogbn-proteins/models.py:159-160;
    `rst + res_fc(h)`, models.py:558-560) instead of a separate pass; its gradient is the incoming one.
    The gradient of an entry of `a` that is exactly 0 comes back as 0 while the sweeps' zero-weight skip is on (the default,
    `_C.spmm_set_zero_skip`): right for weights that a dropout mask zeroed, whose gradient the mask zeroes again; a caller that
    needs the true gradient at a zero weight switches the skip off."""
    return _UMulESum.apply(g, x, a, order, addend)


class _CopyESum(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, w):
        ctx.g, ctx.shape = g, w.shape
        return _C.segment_sum(g.csc, _edge2(w), g.csc.eid).view((g.number_of_dst_nodes(),) + tuple(w.shape[1:]))

    @staticmethod
    def backward(ctx, dout):
        g = ctx.g
        return None, _C.u_add_v(g.dst32, None, _flat2(dout).contiguous()).view(ctx.shape)


def copy_e_sum(g, w):
    """`update_all(fn.copy_e('feat','m'), fn.sum('m','feat'))` — ogbn-proteins/gat.py:58."""
    return _CopyESum.apply(g, w)


class _UAddV(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, x, y):
        ctx.g, ctx.xshape = g, x.shape
        ctx.has_y = y is not None
        ctx.yshape = y.shape if ctx.has_y else None
        x2 = _flat2(x)
        y2 = None if y is None else _flat2(y)
        return _C.u_add_v(g.src32, g.dst32 if ctx.has_y else None, x2, y2).view((g.number_of_edges(),) + tuple(x.shape[1:]))

    @staticmethod
    def backward(ctx, de):
        g = ctx.g
        de2 = _flat2(de).contiguous()
        dx = _C.segment_sum(g.csr, de2, g.csr.eid).view(ctx.xshape) if ctx.needs_input_grad[1] else None
        dy = _C.segment_sum(g.csc, de2, g.csc.eid).view(ctx.yshape) if ctx.has_y and ctx.needs_input_grad[2] else None
        return None, dx, dy


def copy_u(g, x):
    """`apply_edges(fn.copy_u('el','e'))` — models.py:525."""
    return _UAddV.apply(g, x, None)


def u_add_v(g, x, y):
    """`apply_edges(fn.u_add_v('el','er','e'))` — models.py:523."""
    return _UAddV.apply(g, x, y)


class _EdgeMLP(torch.autograd.Function):
    @staticmethod
    def forward(ctx, ef_csc, W1, b1, W2):
        ctx.save_for_backward(ef_csc, W1, b1, W2)
        return _C.edge_mlp_fwd(ef_csc, W1, b1, W2)

    @staticmethod
    def backward(ctx, dz):
        ef_csc, W1, b1, W2 = ctx.saved_tensors
        dW1, db1, dW2 = _C.edge_mlp_bwd(ef_csc, W1, b1, W2, dz.contiguous())
        return None, dW1, db1, dW2


def edge_features_csc(g, efeat):
    """Edge features permuted once into CSC position order (they are constant inputs of the model)."""
    cache = getattr(g, "_bot_cache", None)
    if cache is None:
        cache = g._bot_cache = {}
    key = ("ef_csc", efeat.data_ptr(), efeat._version, tuple(efeat.shape))
    hit = cache.get(key)
    if hit is None or hit[0]() is not efeat:        # (an address is reused once its tensor is freed: the entry must be this very tensor's)
        hit = cache[key] = (weakref.ref(efeat), take_rows(efeat, g.csc.eid).contiguous())
    return hit[1]


def edge_mlp(g, efeat, W1, b1, W2):
    """`attn_edge_fc(relu(edge_encoder(efeat)))` of the ogbn-proteins layer (src/ogbn-proteins/models.py:244-248, :130-131)
    evaluated per edge in registers; returns the logit term [E,H] in CSC position order (use with
    `gat_attention(..., ee=..., ee_order="csc")`).  efeat [E,8] is an input (no gradient), W1 [16,8], b1 [16], W2 [H,16]."""
    return _EdgeMLP.apply(edge_features_csc(g, efeat), W1, b1, W2)


class _GatAttention(torch.autograd.Function):
    @staticmethod
    def forward(ctx, g, el, er, ee, keep, slope, order, ee_csc=False, keep_csc=False):
        csc = g.csc
        H = _flat2(el if el is not None else ee).shape[1]
        el2 = None if el is None else el.reshape(-1, H)
        er2 = None if er is None else er.reshape(-1, H)
        ee2 = None if ee is None else ee.reshape(-1, H)
        aperm = csc.eid if order == "eid" else None
        # one permutation (`eperm`) serves both edge-indexed inputs, so they must be in the same order
        if keep is not None and ee is not None and keep_csc != ee_csc:
            if keep_csc:
                raise ValueError("gat_attention: a CSC-ordered keep mask needs CSC-ordered (or no) edge logits")
            keep = take_rows(keep, csc.eid).contiguous()
        in_csc = ee_csc if ee is not None else keep_csc
        eperm = csc.eid if ((ee is not None or keep is not None) and not in_csc) else None
        zs = _C.zsign_buffer(csc, H, slope)
        a = _C.gat_attn_fwd(csc, el2, er2, ee2, eperm, keep, slope, H, aperm, zs)
        ctx.g, ctx.slope, ctx.order, ctx.H, ctx.ee_csc = g, slope, order, H, ee_csc
        ctx.shapes = tuple(None if t is None else t.shape for t in (el, er, ee))
        ctx.zs = zs
        ctx.save_for_backward(el2, er2, ee2, a)
        return a.view(-1, H, 1)

    @staticmethod
    def backward(ctx, da):
        g, H = ctx.g, ctx.H
        csc, csr = g.csc, g.csr
        el2, er2, ee2, a = ctx.saved_tensors
        aperm = csc.eid if ctx.order == "eid" else None
        eperm = csc.eid if (ee2 is not None and not ctx.ee_csc) else None
        # dz is written in edge-id order when something edge-indexed consumes it, else CSC position order
        z_eid = ee2 is not None and not ctx.ee_csc
        dz, der = _C.gat_attn_bwd(csc, el2, er2, ee2, eperm, ctx.slope, H, a, da.reshape(-1, H), aperm,
                                  csc.eid if z_eid else None, er2 is not None, ctx.zs)
        d_el = d_er = d_ee = None
        if el2 is not None and ctx.needs_input_grad[1]:
            d_el = _C.segment_sum(csr, dz, csr.eid if z_eid else g.csr2csc).view(ctx.shapes[0])
        if er2 is not None and ctx.needs_input_grad[2]:
            d_er = der.view(ctx.shapes[1])
        if ee2 is not None and ctx.needs_input_grad[3]:
            d_ee = dz.view(ctx.shapes[2])
        return None, d_el, d_er, d_ee, None, None, None, None, None


def gat_attention(g, el=None, er=None, ee=None, *, keep=None, negative_slope=0.2, order="eid", ee_order="eid", keep_order="eid"):
    """Attention weights of one GAT layer in a single sweep over the in-edges (models.py:517-544):

        z_e = el[src] (+ er[dst]) (+ ee_e);  a = softmax over in-edges of leaky_relu(z, negative_slope)

    el, er: [N,H,1]; ee: [E,H,1] in edge-id order; keep: optional uint8 [E] in edge-id order — edges
    with keep == 0 are excluded from the softmax and get a == 0 (the edge-drop branch, models.py:528-539).
    `ee_order="csc"`: `ee` is already in CSC position order (what `edge_mlp` returns); `keep_order="csc"` likewise for the mask
    (`random_edge_keep` draws a uniformly random subset, so a layer may use its mask in whichever order is cheapest).
    Returns a [E,H,1] in edge-id order (order="eid") or CSC position order (order="csc")."""
    return _GatAttention.apply(g, el, er, ee, keep, float(negative_slope), order, ee_order == "csc", keep_order == "csc")


def edge_softmax(graph, logits, eids=None, norm_by="dst"):
    """`dgl.ops.edge_softmax(graph, logits, eids=ALL)` — models.py:544 and, with `eids`, :537.

    With `eids`, `logits` holds values for those edges only and the softmax runs over the
    edge-induced subgraph that keeps all nodes; the result has the shape and order of `logits`.

    Non-finite logits: masking by -inf works (such an edge gets weight 0 and the others the softmax without it); a NaN or +inf
    logit makes the weights of its destination and head NaN.  A stated departure from the reference: a destination and head whose
    logits are ALL -inf gets zeros, not NaN."""
    if norm_by != "dst":
        raise NotImplementedError("edge_softmax: only norm_by='dst' is on the reference's path")
    if eids is None or not torch.is_tensor(eids):
        return gat_attention(graph, None, None, logits, negative_slope=1.0, order="eid").view(logits.shape)
    E = graph.number_of_edges()
    full = logits.new_zeros((E,) + tuple(logits.shape[1:])).index_copy(0, eids, logits)
    keep = torch.zeros(E, dtype=torch.uint8, device=logits.device)
    keep[eids] = 1
    a = gat_attention(graph, None, None, full, keep=keep, negative_slope=1.0, order="eid")
    return take_rows(a.view(full.shape), eids)


# ------------------------------------------------------------------------------------------------ fused hidden-layer epilogue
def _dist_group(bn):
    """(do_sync, group) — global statistics when `bn` is a bot_amd.dist.SyncBatchNorm1d and a process group is up."""
    import torch.distributed as dist
    if getattr(bn, "_bot_sync", False) and dist.is_available() and dist.is_initialized() and dist.get_world_size(bn.group) > 1:
        return True, bn.group
    return False, None


def bn_batch_stats(x, bn, bn_training, halves_p=None, partials=None):
    """Column statistics for the fused epilogue: (mean, invstd, total_count, sync, group); updates bn's running statistics
    exactly like nn.BatchNorm1d (momentum, unbiased running variance).  In partitioned mode the (count, mean, M2) triples of
    the ranks are merged with Chan et al.'s pairwise formula through two small all-reduces.
    `halves_p` (the epilogue's dropout rate) asks for a sixth value: the fp16-halves scale of the epilogue's output, derived
    from the column extremes in the same pass (bot_bn_stats_halves_f32) — None where that call does not apply (partitioned
    statistics, eval mode)."""
    import torch.distributed as dist
    n = x.shape[0]
    sync, group = _dist_group(bn)
    total = float(n)
    extra = () if halves_p is None else (None,)
    if not bn_training:
        return (bn.running_mean, torch.rsqrt(bn.running_var + bn.eps), total, sync, group) + extra
    if not sync and (bn.momentum is not None or not bn.track_running_stats):
        # one GPU: statistics, invstd and the running-statistics update in ONE call (nine elementwise launches per layer before)
        track = bn.track_running_stats
        args = (x, bn.eps, bn.momentum if track else 0.0, bn.running_mean if track else None, bn.running_var if track else None,
                bn.num_batches_tracked if track else None)
        with torch.no_grad():
            if halves_p is not None and partials is not None:
                # the producer of x delivered the column partials with it (`stats_partials_for`): no pass over x
                part, minmax, pivot = partials
                mean, invstd, hscale = _C.bn_stats_halves_partials(part, minmax, pivot, n, *args[1:], bn.weight, bn.bias, halves_p)
                return mean, invstd, total, sync, group, hscale
            if halves_p is not None:
                mean, invstd, hscale = _C.bn_stats_halves(*args, bn.weight, bn.bias, halves_p)
                return mean, invstd, total, sync, group, hscale
            mean, invstd = _C.bn_stats(*args)
        return mean, invstd, total, sync, group
    mean, m2 = _C.colstats(x)
    if sync:
        # the global row count is a constant of the partition: ask for it once (one host sync), then never again, so the
        # host keeps running ahead of the GPU during the step
        totals = bn.__dict__.setdefault("_bot_total_rows", {})
        key = (id(group), dist.get_rank(group), n)   # per process group and local row count (one partition per rank and group)
        if key not in totals:
            cnt = mean.new_full((1,), float(n))
            dist.all_reduce(cnt, group=group)
            totals[key] = float(cnt.item())
        total = totals[key]
        gmean = mean * (n / total)
        dist.all_reduce(gmean, group=group)
        m2 = m2 + n * (mean - gmean) ** 2
        dist.all_reduce(m2, group=group)
        mean = gmean
    invstd = torch.rsqrt(m2 / total + bn.eps)
    if bn.track_running_stats:
        with torch.no_grad():
            bn.num_batches_tracked += 1
            # nn.BatchNorm1d: momentum None = cumulative moving average, factor 1 / num_batches_tracked (one host read per
            # step in that rarely used mode)
            mom = 1.0 / float(bn.num_batches_tracked) if bn.momentum is None else bn.momentum
            bn.running_mean.mul_(1 - mom).add_(mean, alpha=mom)
            bn.running_var.mul_(1 - mom).add_(m2 / max(total - 1.0, 1.0), alpha=mom)
    return (mean, invstd, total, sync, group) + extra


STATS_BYPRODUCT = os.environ.get("BOT_STATS_BYPRODUCT", "1") != "0"


def stats_partials_for(bn, bn_training, n_rows, F, device, halves_ok):
    """Buffers for a producer that can deliver BatchNorm's column partials as a by-product (the grouped NT GEMM's epilogue), or None when
    `bn_batch_stats` would not take them (eval mode, partitioned statistics, no halves epilogue): (part, minmax, pivot), all written by the
    producer.  The shift of a 256-row tile's sums is the tile's own FIRST value (ABI 19; round 5 shifted by zero, which lost
    (mean / std)^2 ulps of the variance on un-centred columns): a state-independent choice inside the data; the finish re-bases
    the tiles onto the first tile's pivot exactly, in double (csrc/dense.hip colstats_tiles_final_kernel)."""
    sync, _ = _dist_group(bn)
    if not (STATS_BYPRODUCT and bn_training and halves_ok and not sync and (bn.momentum is not None or not bn.track_running_stats)):
        return None
    tiles = (n_rows + 255) // 256
    return (torch.empty((tiles, 2, F), dtype=torch.float32, device=device), torch.empty((tiles, 2, F), dtype=torch.float32, device=device),
            torch.empty((tiles, F), dtype=torch.float32, device=device))


def random_edge_keep(graph, drop):
    """Edge-drop mask of one training step (models.py:528-532: `perm = randperm(E); eids = perm[int(E * drop):]`): uint8
    [E], 1 for a uniformly random subset of exactly E - int(E * drop) edges.  The seed comes from torch's CPU generator."""
    E = graph.number_of_edges()
    return _C.random_keep(E, E - int(E * drop), new_dropout_seed(1.0), graph.device)


def new_dropout_seed(p):
    """Seed of the Philox stream of one fused-dropout call, drawn from torch's CPU generator (so torch.manual_seed governs it)."""
    return int(torch.empty((), dtype=torch.int64).random_().item()) if p > 0 else 0


MODULAR_BN_LINK = os.environ.get("BOT_BN_LINK_MODULAR", "1") != "0"     # the modular epilogue (GCN, the edge-GAT stacks) takes part in gemm.BnLink too


# The non-tensor state a BatchNorm / ReLU / dropout epilogue keeps on ctx for its backward (its tensors go to save_for_backward).
# out_link: a gemm.BnLink (the consumer's `d h` product may deliver the backward's reduce pass) or None.
BnEpilogue = namedtuple("BnEpilogue", "drop_p seed bn_training sync group total out_link")


def bn_epilogue_forward(x, bn, weight, bias, relu, p, bn_training, halves, link, y_needed=True, partials=None):
    """BatchNorm statistics + the fused BatchNorm / ReLU / dropout pass -> (y, mean, invstd, BnEpilogue).  `halves`: when the next
    projection runs on fp16 halves (bot_amd.gemm) the pass writes them too (gemm.take picks them up) and the scale comes from the
    statistics pass; `link`: such halves carry a gemm.BnLink.  `partials`: the kernel that wrote x delivered BatchNorm's column partials
    with it (no statistics pass over x).  y_needed=False: see bot_amd.nn.fused._epilogue_forward."""
    from . import gemm
    seed = new_dropout_seed(p)
    piece = gemm.epilogue_piece(x.shape[1], x) if halves and bn_training else None
    hscale = out_link = None
    if piece is not None:
        mean, invstd, total, sync, group, hscale = bn_batch_stats(x, bn, bn_training, halves_p=p, partials=partials)
    else:
        mean, invstd, total, sync, group = bn_batch_stats(x, bn, bn_training)
    if hscale is not None:
        order = gemm.left_order(piece)
        y, buf = _C.bn_act_fwd(x, mean, invstd, weight, bias, relu, p, seed, halves=(hscale, piece, 2 if order == 2 else 3), want_y=y_needed)
        if y is None:
            y = gemm.make_handle(x, x.shape[0], x.shape[1])
        hv = gemm.Halves(buf, hscale, x.shape[0], x.shape[1], piece, order)
        # the consumer's backward can deliver this epilogue's reduce pass with the gradient it sends back (gemm.BnLink)
        hv.bn_link = out_link = gemm.BnLink(x, mean, invstd, weight, bias, p, seed, relu=relu, sync=sync) if (link and gemm.BN_BYPRODUCT) else None
        gemm.stash(y, hv)
    else:
        y = _C.bn_act_fwd(x, mean, invstd, weight, bias, relu, p, seed)
    return y, mean, invstd, BnEpilogue(p, seed, bn_training, sync, group, total, out_link)


def bn_epilogue_sums(epi, dy, x, mean, invstd, weight, bias, relu, all_reduce, slots=None):
    """Column sums of the epilogue's backward -> (the apply pass's (sum_g, sum_gx), (None, None) under running statistics; this rank's
    (sum_g, sum_gx), i.e. d bias / d weight: the ranks' parameter gradients are summed later with all the others).  `dy` may be a deferred
    gradient (gemm.DeferredDh: an unwritten handle, recognised by the caller BEFORE any `.contiguous()`): it is only identified here, never read
    - the reduce pass that would read it runs only when there are no partials for it, and a deferred gradient always has them.  From the partials
    the consumer's `d h` product delivered with `dy` (gemm.BnLink, claimed here) if there are any for exactly this tensor, else by the
    reduce pass.  all_reduce: sum the apply pass's sums over `epi.group` (sync BatchNorm).  slots: also fold a bound on max|dx| into
    them, from the column maxima and the final sums (bot_bn_bwd_bound_f32)."""
    import torch.distributed as dist
    train, total = epi.bn_training, epi.total
    st = epi.out_link.claim(dy) if epi.out_link is not None else None
    if st is not None and slots is not None and not all_reduce:          # one rank: the partials are finished in ONE launch
        sg, sgx = st.finish(train, total, slots)
        return ((sg, sgx) if train else (None, None)), (sg, sgx)
    if st is not None:
        sg, sgx = st.sums()
    elif slots is not None:
        sg, sgx, ws = _C.bn_act_bwd_reduce(dy, x, mean, invstd, weight, bias, relu, epi.drop_p, epi.seed, want_max=True)
    else:
        sg, sgx = _C.bn_act_bwd_reduce(dy, x, mean, invstd, weight, bias, relu, epi.drop_p, epi.seed)
    local = sg, sgx
    if all_reduce:
        both = torch.stack([sg, sgx])
        dist.all_reduce(both, group=epi.group)
        sg, sgx = both[0].contiguous(), both[1].contiguous()
    sums = (sg, sgx) if train else (None, None)
    if slots is not None and st is not None:
        st.bound(*sums, total, slots)
    elif slots is not None:
        _C.bn_bwd_bound(ws, dy.shape[0], *sums, total, weight, invstd, slots)
    return sums, local


class _BNActDrop(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, bn, relu, p, bn_training, halves=False):
        y, mean, invstd, ctx.epi = bn_epilogue_forward(x, bn, weight, bias, relu, p, bn_training, halves, MODULAR_BN_LINK)
        ctx.save_for_backward(x, mean, invstd, weight, bias)
        ctx.relu = relu
        return y

    @staticmethod
    def backward(ctx, dy):
        x, mean, invstd, weight, bias = ctx.saved_tensors
        epi, relu = ctx.epi, ctx.relu
        if epi.out_link is not None:
            dy = epi.out_link.stored(dy)        # (a deferred gradient - gemm.DeferredDh - is formed first: this node has no fused apply step)
        dy = dy.contiguous()
        want_dx = ctx.needs_input_grad[0]
        (sg, sgx), (lg, lgx) = bn_epilogue_sums(epi, dy, x, mean, invstd, weight, bias, relu, want_dx and epi.bn_training and epi.sync)
        dw = lgx if weight is not None and ctx.needs_input_grad[1] else None
        db = lg if bias is not None and ctx.needs_input_grad[2] else None
        dx = _C.bn_act_bwd_apply(dy, x, mean, invstd, weight, bias, relu, epi.drop_p, epi.seed, sg, sgx, epi.total) if want_dx else None
        return dx, dw, db, None, None, None, None, None


class _AddBias(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, b):
        return x + b

    @staticmethod
    def backward(ctx, dy):
        db = None
        if ctx.needs_input_grad[1]:
            db = _C.colsum(dy)                 # column sums by the tree-reduction kernel of the BatchNorm statistics
        return dy, db


def add_bias(x, b):
    """x [N,F] + b [F] with the bias gradient computed by the column-statistics kernel."""
    return _AddBias.apply(x, b) if x.dim() == 2 and x.is_cuda == b.is_cuda else x + b


class _SumAll(torch.autograd.Function):
    """Sum of all entries of a float32 CUDA tensor through bot_colsum_f32: the tensor is viewed as [n / 64, 64], the column sums
    are taken by the two-stage tree kernel (finished in double, fixed order) and the <= 127 leftovers by a single-workgroup reduce.

    Why not `x.sum()`: torch's multi-workgroup reductions (a staging buffer + a semaphore zeroed by a memset in front of the kernel)
    give WRONG results inside a replayed hipGraph on this stack — measured in round 3 on the final bias gradient of the GAT stack
    (`dy.sum(0)` over [N, 40]): bit-identical to the eager step for the first replays, then off by ~1e-1 of the gradient on every
    further replay, identical in every run (tools/dbg_captured_eval.py); the same step with `bot_colsum_f32` matches the eager step bit for
    bit over any number of replays.  The train step (bot_amd.train / bot_amd.dist) therefore takes its N-sized reductions — the loss
    numerator, the weight count, bias gradients — through the library's own deterministic kernels."""

    @staticmethod
    def forward(ctx, x):
        ctx.shape = x.shape
        flat = x.reshape(-1)
        n64 = flat.numel() // 64 * 64
        parts = []
        if n64:
            parts.append(_C.colsum(flat[:n64].view(-1, 64)))
        if n64 < flat.numel():
            parts.append(flat[n64:])
        return torch.cat(parts).sum() if parts else flat.sum()

    @staticmethod
    def backward(ctx, g):
        return g.expand(ctx.shape)


def sum_all(x):
    """x.sum() with a fixed summation order that is also safe under hipGraph replay (see _SumAll); plain x.sum() off the GPU."""
    return _SumAll.apply(x) if (x.is_cuda and x.dtype == torch.float32 and x.numel() >= 4096) else x.sum()


SPLITK_MIN_ROWS = 1 << 20      # weight gradients over at least this many rows are reduced in row chunks
SPLITK_CHUNK_ROWS = 1 << 14


def weight_grad(dy, x):
    """dy^T x ([P,N] x [N,K]) — the weight gradient of a Linear, a reduction over all N rows.  From 2^20 rows on it is computed
    as N / 2^14 partial products over row chunks (ONE batched GEMM) summed afterwards: at S-products (N = 2.45 M, P = K = 480)
    the single GEMM's fp32 accumulation is 1.0e-4 of the largest entry away from the fp64 product, the chunked one 1.3e-6 to
    5e-6, and it is faster (8.7 vs 9.7 ms; tools/exp_splitk_dw.py).  The pre-BatchNorm gradients make this reduction
    cancellation-heavy (their column sums are zero), which is why the accumulation order shows."""
    n = x.shape[0]
    if n < SPLITK_MIN_ROWS or not dy.is_contiguous() or not x.is_contiguous():
        return dy.t() @ x
    S = n // SPLITK_CHUNK_ROWS
    R = n // S
    dw = torch.bmm(dy[:S * R].view(S, R, -1).transpose(1, 2), x[:S * R].view(S, R, -1)).sum(0)
    if S * R < n:
        dw = dw + dy[S * R:].t() @ x[S * R:]
    return dw


class _MatmulT(torch.autograd.Function):
    """y = x W^T with the weight gradient through `weight_grad`."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return torch.mm(x, w.t())

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dx = torch.mm(dy, w) if ctx.needs_input_grad[0] else None
        dw = weight_grad(dy.contiguous(), x) if ctx.needs_input_grad[1] else None
        return dx, dw


def linear(x, weight, bias=None):
    """`F.linear` for [N, K] inputs whose two all-row reductions are done carefully: the bias gradient (a column sum over N
    rows) runs on the colstats kernel — the stock reduction takes 19 ms for [2 449 029, 47] (S-products classifier,
    ogbn-products/models.py:262), longer than the classifier GEMMs — and the weight gradient goes through `weight_grad`."""
    from . import gemm
    y = gemm.linear(x, weight)                                          # on the fp16 matrix cores where the shapes pay
    if y is None:
        y = _MatmulT.apply(x, weight) if x.shape[0] >= SPLITK_MIN_ROWS and torch.is_grad_enabled() else torch.mm(x, weight.t())
    return y if bias is None else _AddBias.apply(y, bias)


def bn_relu_dropout(x, bn, *, relu=True, p=0.0, training=False, halves=False):
    """`dropout(relu(bn(x)))` over the node axis in 2 reads + 1 write (models.py:636-639, :726-731).

    `bn` is the layer's nn.BatchNorm1d (its parameters, running statistics and train/eval state are used and
    updated exactly as nn.BatchNorm1d would); `p` is the dropout rate, applied when `training`."""
    w = bn.weight if bn.affine else None
    b = bn.bias if bn.affine else None
    bn_training = bn.training or not bn.track_running_stats
    return _BNActDrop.apply(x, w, b, bn, bool(relu), float(p) if training else 0.0, bn_training, bool(halves))


from .appnp import appnp_keep, appnp_propagate  # noqa: E402 - appnp.py draws its seeds from new_dropout_seed above
