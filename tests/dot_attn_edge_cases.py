"""Float64 restatements of dot-product attention with edge features (include/bot_gnn.h "Dot-product attention with edge features";
`ops.dot_attention_edge`), shared by tests/test_dot_attn_edge_host.py and tests/test_dot_attn_edge_gpu.py.  Nothing here calls the
code under test, except `check_op` at the end.  Built on tests/dot_attn_cases.py, which stays as it is.

Two levels.  OP level, written PyG's way (`attention64`): project the raw features, E = (ef W^T).view(E, H, D), add E to the gathered
key and value rows, softmax, dropout, sum.  KERNEL level (`forward64` / `backward64`): what the sweeps are handed - a GIVEN float32
qe [n_dst, H, K] beside q, k, v and position-ordered ef - and what they return: out, lse, aef and dq, dqe, p, ds (dk and dv through the
plain sweep over the sources).

Bounds, derived as tests/dot_attn_cases.py derives its own (and with its constants U and EXP_ERR):
  kernel level  the logit is a rounded sum of D + K products, so its rounding is (D + K + 3) U scale (sum_d |q k| + sum_j |qe ef|);
                everything downstream of the logit is dot_attn_cases' form with that eps.  aef and dqe are sequential sums like out and
                dq with |ef| in place of |v| and |k|, two roundings per term.  delta and dd gain K products: (D + K + 5) U of their
                absolute terms, and delta also moves with aef (sum_j |daef| aef_bound).
  op level      qe = q W and daef = dout W are float32 products of D terms formed in front of the sweeps: each entry carries (D + 2) U of
                its absolute terms, which moves the logit by scale sum_j that |ef_j| and dd by the same form.  Both are covered by
                taking the absolute terms of the edge part as sum_d |q_d| sum_j |W_dj ef_j| (>= |qe ef|) and (2 D + K + 5) U for
                (D + K + 3) U.  The result adds W aef, K terms: sum_j |W| aef_bound + (K + 2) U (|out| + sum_j |W aef|); dq adds dqe W in
                the same way, and dW[h, d, j] = sum_v (q dqe + dout aef) is a sum over n_dst rows: the terms' own errors and
                (n_dst + 3) U of their absolute values."""
import numpy as np
import torch

from tests import dot_attn_cases as DC
from tests.dot_attn_cases import EXP_ERR, F64, U, degree_of, positions  # noqa: F401

_tot = DC._tot


# ------------------------------------------------------------------------------------------------ op level, PyG's way
def attention64(src, dst, n_dst, q, k, v, ef, W, scale, keep=None, c=1.0):
    """PyG's TransformerConv(edge_dim=K) message passing as differentiable float64 torch: ef [E, K] row per (src, dst) entry, W
    [H * D, K] as nn.Linear stores it.  -> out [n_dst, H, D]."""
    H, D = q.shape[1], q.shape[2]
    E = (ef @ W.t()).view(-1, H, D)                                        # project
    key, val = k[src] + E, v[src] + E                                      # add to key and value
    s = (q[dst] * key).sum(-1) * scale
    idx = dst.view(-1, 1).expand(-1, H)
    m = torch.full((n_dst, H), -np.inf, dtype=s.dtype).scatter_reduce(0, idx, s.detach(), "amax", include_self=True)
    ex = torch.exp(s - m[dst])
    den = torch.zeros((n_dst, H), dtype=s.dtype).index_add(0, dst, ex)
    a = ex / den[dst]                                                      # softmax
    w = a if keep is None else a * keep.to(a.dtype) * c                    # dropout
    return torch.zeros((n_dst, H, D), dtype=v.dtype).index_add(0, dst, w.unsqueeze(-1) * val)     # sum


def op_backward64(src, dst, n_src, n_dst, q, k, v, ef, W, scale, dout, keep=None, c=1.0):
    """The analytic gradients of `attention64` for q, k, v, W and ef (`def_`, one row per (src, dst) entry) (float64 tensors in, a dict out)."""
    H, D = q.shape[1], q.shape[2]
    K = ef.shape[1]
    W3 = W.view(H, D, K)
    qe = torch.einsum("nhd,hdk->nhk", q, W3)
    fwd = forward64(src, dst, n_dst, q, k, v, ef, qe, scale, keep, c)
    daef = torch.einsum("nhd,hdk->nhk", dout, W3)
    bwd = backward64(src, dst, n_src, n_dst, q, k, v, ef, qe, scale, dout, daef, fwd, keep, c)
    dW = torch.einsum("nhd,nhk->hdk", q, bwd["dqe"]) + torch.einsum("nhd,nhk->hdk", dout, fwd["aef"])
    dE = scale * bwd["ds"].unsqueeze(-1) * q[dst] + bwd["p"].unsqueeze(-1) * dout[dst]          # d E_e [E, H, D]: through the key and the value
    return dict(def_=torch.einsum("ehd,hdk->ek", dE, W3), dq=bwd["dq"] + torch.einsum("nhk,hdk->nhd", bwd["dqe"], W3), dk=bwd["dk"], dv=bwd["dv"], dW=dW.reshape(H * D, K),
                out=fwd["out"] + torch.einsum("nhk,hdk->nhd", fwd["aef"], W3), fwd=fwd, bwd=bwd, qe=qe, daef=daef)


# ------------------------------------------------------------------------------------------------ kernel level
def forward64(src, dst, n_dst, q, k, v, ef, qe, scale, keep=None, c=1.0, eabs=None):
    """The forward contract in float64 with a GIVEN qe [n_dst, H, K]: `dot_attn_cases.forward64`'s dict (out WITHOUT the edge term's
    projection) plus aef [n_dst, H, K] and efmax.  sabs counts the edge products too; `eabs` [E, H]: the edge part's absolute terms
    where the caller knows a larger one (the op level)."""
    H = q.shape[1]
    s = ((q[dst] * k[src]).sum(-1) + (qe[dst] * ef.unsqueeze(1)).sum(-1)) * scale
    if eabs is None:
        eabs = (qe[dst] * ef.unsqueeze(1)).abs().sum(-1)
    sabs = ((q[dst] * k[src]).abs().sum(-1) + eabs) * abs(scale)
    idx = dst.view(-1, 1).expand(-1, H)
    deg = degree_of(dst, n_dst)
    m = torch.zeros((n_dst, H), dtype=F64).scatter_reduce(0, idx, s, "amax", include_self=False)
    ex = torch.exp(s - m[dst])
    den = torch.zeros((n_dst, H), dtype=F64).index_add_(0, dst, ex)
    some = (deg > 0).view(-1, 1)
    lse = torch.where(some, m + torch.log(torch.where(some, den, torch.ones((), dtype=F64))), torch.zeros((), dtype=F64))
    a = ex / den[dst]
    w = a if keep is None else a * keep.to(F64) * c
    out = _tot(n_dst, dst, w.unsqueeze(-1) * v[src])
    aef = _tot(n_dst, dst, w.unsqueeze(-1) * ef.unsqueeze(1))
    amax = lambda t: torch.zeros((n_dst,) + tuple(t.shape[1:]), dtype=F64).scatter_reduce(
        0, dst.view((-1,) + (1,) * (t.dim() - 1)).expand_as(t), t, "amax", include_self=True)
    return dict(out=out, aef=aef, lse=lse, a=a, w=w, s=s, deg=deg, sabs=sabs, vmax=amax(v[src].abs()),
                efmax=amax(ef.abs().unsqueeze(1).expand(-1, H, -1).contiguous()), smax=amax(s.abs()), sabs_max=amax(sabs))


def backward64(src, dst, n_src, n_dst, q, k, v, ef, qe, scale, dout, daef, fwd, keep=None, c=1.0, ddabs_e=None, delabs_e=None):
    """The analytic gradients of the kernel-level contract in float64: dq, dqe, dk, dv, p, ds and the absolute sums the bounds need."""
    a, out, aef = fwd["a"], fwd["out"], fwd["aef"]
    ck = torch.full_like(a, 1.0) if keep is None else keep.to(F64) * c
    e3 = ef.unsqueeze(1)
    delta = (dout * out).sum(-1) + (daef * aef).sum(-1)
    dd = (dout[dst] * v[src]).sum(-1) + (daef[dst] * e3).sum(-1)
    p = ck * a
    ds = a * (ck * dd - delta[dst])
    dq = scale * _tot(n_dst, dst, ds.unsqueeze(-1) * k[src])
    dqe = scale * _tot(n_dst, dst, ds.unsqueeze(-1) * e3)
    dk = scale * _tot(n_src, src, ds.unsqueeze(-1) * q[dst])
    dv = _tot(n_src, src, p.unsqueeze(-1) * dout[dst])
    if ddabs_e is None:
        ddabs_e = (daef[dst] * e3).abs().sum(-1)
    if delabs_e is None:
        delabs_e = (daef * aef).abs().sum(-1)
    return dict(dq=dq, dqe=dqe, dk=dk, dv=dv, p=p, ds=ds, ck=ck, ddabs=(dout[dst] * v[src]).abs().sum(-1) + ddabs_e,
                delabs=(dout * out).abs().sum(-1) + delabs_e)


def forward_bounds(fwd, D, K, c=1.0, logit_terms=None):
    """out, lse (dot_attn_cases.forward_bounds with the logit's D + K products) and aef (out's form over |ef|).  `logit_terms`: the
    count in front of U for the logit's rounding, D + K + 3 at kernel level."""
    n = D + K if logit_terms is None else logit_terms - 3
    fb = DC.forward_bounds(fwd, n, c)
    fb["aef"] = (fb["rel"] + 4 * fb["eps"]).unsqueeze(-1) * c * fwd["efmax"]
    return fb


def backward_bounds(src, dst, n_src, n_dst, q, k, v, ef, scale, dout, daef, fwd, bwd, fb, D, K, c=1.0, rho=None, given=False, dot_terms=None):
    """dq, dqe, dk, dv, p, ds: dot_attn_cases.backward_bounds with delta and dd of D + K products (`dot_terms` + 5 in front of U), delta
    moving with out AND aef, and dqe a sequential sum over the in-edges with two roundings per term."""
    a, ck = fwd["a"], bwd["ck"]
    n = D + K if dot_terms is None else dot_terms
    if rho is None:
        rho = (2 * EXP_ERR + fb["eps"] + fb["lse"] + 2 * U * (fwd["smax"] + fwd["lse"].abs()))[dst]
    mag = ck * bwd["ddabs"] + bwd["delabs"][dst]
    d_err = 0.0 if given else ((dout.abs() * fb["out"]).sum(-1) + (daef.abs() * fb["aef"]).sum(-1))[dst]
    ds_err = a * ((rho + (n + 5) * U) * mag + d_err)
    ds_abs = a * mag
    p_err = ck * a * (rho + 2 * U)
    s = abs(scale)
    deg_in, deg_out = degree_of(dst, n_dst).view(-1, 1, 1), degree_of(src, n_src).view(-1, 1, 1)
    e3 = lambda t: t.unsqueeze(-1)
    efa = ef.abs().unsqueeze(1)
    dq = s * (_tot(n_dst, dst, e3(ds_err) * k[src].abs()) + (deg_in + 4) * U * _tot(n_dst, dst, e3(ds_abs) * k[src].abs()))
    dqe = s * (_tot(n_dst, dst, e3(ds_err) * efa) + (2 * deg_in + 4) * U * _tot(n_dst, dst, e3(ds_abs) * efa))
    dk = s * (_tot(n_src, src, e3(ds_err) * q[dst].abs()) + (deg_out + 4) * U * _tot(n_src, src, e3(ds_abs) * q[dst].abs()))
    dv = _tot(n_src, src, e3(p_err) * dout[dst].abs()) + (deg_out + 3) * U * _tot(n_src, src, e3(bwd["p"]) * dout[dst].abs())
    return dict(dq=dq, dqe=dqe, dk=dk, dv=dv, p=p_err, ds=ds_err + 3 * U * ds_abs)


def op_bounds(src, dst, n_src, n_dst, q, k, v, ef, W, scale, dout, ref, keep=None, c=1.0):
    """The op-level bounds (module docstring) for out, dq, dk, dv, dW from float64 operands and `op_backward64`'s dict."""
    H, D = q.shape[1], q.shape[2]
    K = ef.shape[1]
    W3a = W.view(H, D, K).abs()
    wef = torch.einsum("hdk,ek->ehd", W3a, ef.abs())                        # sum_j |W_dj ef_j| per edge
    eabs = (q[dst].abs() * wef).sum(-1)
    fwd = forward64(src, dst, n_dst, q, k, v, ef, ref["qe"], scale, keep, c, eabs=eabs)
    fb = forward_bounds(fwd, D, K, c, logit_terms=2 * D + K + 5)
    daef = ref["daef"]
    bwd = backward64(src, dst, n_src, n_dst, q, k, v, ef, ref["qe"], scale, dout, daef, fwd, keep, c,
                     ddabs_e=(dout[dst].abs() * wef).sum(-1), delabs_e=torch.einsum("nhd,hdk,nhk->nh", dout.abs(), W3a, fwd["aef"].abs()))
    daef_err = (D + 2) * U * torch.einsum("nhd,hdk->nhk", dout.abs(), W3a)   # the float32 product in front of the backward sweep
    bb = backward_bounds(src, dst, n_src, n_dst, q, k, v, ef, scale, dout, daef.abs() + daef_err, fwd, bwd, fb, D, K, c, dot_terms=2 * D + K)
    proj = lambda t: torch.einsum("nhk,hdk->nhd", t, W3a)
    out = fb["out"] + proj(fb["aef"]) + (K + 2) * U * (fwd["out"].abs() + proj(fwd["aef"].abs()))
    dq = bb["dq"] + proj(bb["dqe"]) + (K + 2) * U * (bwd["dq"].abs() + proj(bwd["dqe"].abs()))
    dW = (torch.einsum("nhd,nhk->hdk", q.abs(), bb["dqe"]) + torch.einsum("nhd,nhk->hdk", dout.abs(), fb["aef"])
          + (n_dst + 3) * U * (torch.einsum("nhd,nhk->hdk", q.abs(), bwd["dqe"].abs()) + torch.einsum("nhd,nhk->hdk", dout.abs(), fwd["aef"].abs())))
    # d ef[e, j] = sum_hd W[hd, j] (scale ds q + p dout): the terms' own errors and, for a sum of H D terms of five roundings each formed in
    # any order, (H D + 8) U of their absolute values
    dE_err = abs(scale) * bb["ds"].unsqueeze(-1) * q[dst].abs() + bb["p"].unsqueeze(-1) * dout[dst].abs()
    dE_abs = abs(scale) * bwd["ds"].abs().unsqueeze(-1) * q[dst].abs() + bwd["p"].unsqueeze(-1) * dout[dst].abs()
    def_ = torch.einsum("ehd,hdk->ek", dE_err + (H * D + 8) * U * dE_abs, W3a)
    return dict(out=out, dq=dq, dk=bb["dk"], dv=bb["dv"], dW=dW.reshape(H * D, K), def_=def_)


# ------------------------------------------------------------------------------------------------ inputs
def eid_of_positions(g):
    """The edge id of every CSC position (int64 CPU): the row of an edge-id-ordered tensor that position reads."""
    from bot_amd.ops import _csc_edge_rows
    rows = _csc_edge_rows(g)
    return torch.arange(g.number_of_edges()) if rows is None else rows.cpu().long()


def normal_inputs(n_src, n_dst, E, H, D, K, seed):
    """q, k, v, dout as dot_attn_cases.normal_inputs; ef [E, K], W [H * D, K] scaled like nn.Linear's, and a float32 qe, daef pair for
    the kernel level."""
    q, k, v, dout = DC.normal_inputs(n_src, n_dst, H, D, seed)
    gen = torch.Generator().manual_seed(seed + 1000)
    ef = torch.randn(E, K, generator=gen)
    W = torch.randn(H * D, K, generator=gen) * K ** -0.5
    qe, daef = torch.randn(n_dst, H, K, generator=gen), torch.randn(n_dst, H, K, generator=gen)
    return q, k, v, dout, ef, W, qe, daef


def check_op(g, dev, H, D, K, seed, impl=None, p=0.0, worst=None, ef_grad=False):
    """`ops.dot_attention_edge` forward and the gradients of q, k, v, weight - with `ef_grad` also ef's, which only the tensor form has -
    on seeded normal inputs against PyG's formula in float64 under the op-level bounds -> (results, bounds).  ef is handed in EDGE-ID
    order."""
    from bot_amd import ops
    src, dst = positions(g)
    n_src, n_dst, E = g.number_of_src_nodes(), g.number_of_dst_nodes(), src.numel()
    q, k, v, dout, ef, W, _, _ = normal_inputs(n_src, n_dst, E, H, D, K, seed)
    ef_pos = ef[eid_of_positions(g)]
    keep = DC.draw_keep(E, H, p, seed + 1) if p > 0 else None
    c = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    sc = D ** -0.5
    a64 = [t.double() for t in (q, k, v, ef_pos, W)]
    ref = op_backward64(src, dst, n_src, n_dst, *a64, sc, dout.double(), keep, c)
    lim = op_bounds(src, dst, n_src, n_dst, *a64, sc, dout.double(), ref, keep, c)
    ql, kl, vl, Wl = (t.clone().to(dev).requires_grad_() for t in (q, k, v, W))
    efl = ef.clone().to(dev).requires_grad_(ef_grad)
    out = ops.dot_attention_edge(g, ql, kl, vl, efl, Wl, keep=None if keep is None else keep.to(dev), p=p, impl=impl)
    assert out.shape == (n_dst, H, D) and out.dtype == torch.float32
    out.backward(dout.to(dev))
    got = dict(out=out.detach(), dq=ql.grad, dk=kl.grad, dv=vl.grad, dW=Wl.grad)
    got = {n: t.cpu().double() for n, t in got.items()}
    if ef_grad:                                                  # (the tensor form's: in edge-id order; the restatement's rows are positions)
        got["def_"] = efl.grad.cpu().double()[eid_of_positions(g)]
    for name in got:
        err = (got[name] - ref[name]).abs()
        frac = float((err / lim[name].clamp(min=1e-300)).max()) if err.numel() else 0.0
        if worst is not None:
            worst[name] = max(worst.get(name, 0.0), frac)
        assert bool((err <= lim[name]).all()), (name, H, D, K, impl, frac)
    return got, lim


# ------------------------------------------------------------------------------------------------ the layer and the stack, float64
def edge_transformer_conv64(conv, src, dst, n_dst, x_src, x_dst, p, ef, keep=None):
    """`EdgeTransformerConv` in float64; ef [E, K] float64, one row per (src, dst) entry."""
    H, C = conv.heads, conv.out_channels
    q, k, v = (DC._lin(x, p, n).view(-1, H, C) for x, n in ((x_dst, "lin_query"), (x_src, "lin_key"), (x_src, "lin_value")))
    out = attention64(src, dst, n_dst, q, k, v, ef, p["lin_edge.weight"], C ** -0.5, keep, 1.0 if keep is None else 1.0 / (1.0 - conv.dropout))
    out = out.reshape(-1, H * C) if conv.concat else out.mean(1)
    if conv.root_weight:
        x_r = DC._lin(x_dst, p, "lin_skip")
        if conv.lin_beta is not None:
            b = torch.sigmoid(torch.cat([out, x_r, out - x_r], dim=-1) @ p["lin_beta.weight"].t())
            out = b * x_r + (1 - b) * out
        else:
            out = out + x_r
    return out


def edge_unimp_stack64(model, layers, feat, p):
    """`EdgeUniMP` in eval mode in float64; layers: per layer (src, dst, n_dst, ef float64 in the order of src / dst)."""
    h = feat
    n = len(model.convs)
    for i, (src, dst, n_dst, ef) in enumerate(layers):
        h = edge_transformer_conv64(model.convs[i], src, dst, n_dst, h, h[:n_dst], DC.layer_params(p, i), ef)
        if i < n - 1:
            if len(model.norms):
                bn = model.norms[i]
                h = (h - bn.running_mean.cpu().double()) * torch.rsqrt(bn.running_var.cpu().double() + bn.eps) * p[f"norms.{i}.weight"] + p[f"norms.{i}.bias"]
            h = torch.relu(h)
    return h


# ------------------------------------------------------------------------------------------------ the one-hot regime with an edge term
def onehot_inputs(g, H, D, K, seed, lim=None, elim=2, keep=None, c=1.0):
    """`dot_attn_cases.onehot_inputs` with an integer edge term: integer-valued q, k, qe, ef and scale = 128, so two logits of a row are
    equal or at least 128 apart and every weight is 0 or 1 / (number of maximal in-edges).  k[u, h, 0] = (u + 1) (2 (lim^2 (D - 1) + R) +
    1) with R = K * 2 * elim the range of the edge term (qe in {-2, -1, 1, 2}, ef in [-elim, elim]) and q[v, h, 0] = +-1: two DISTINCT
    sources never tie (where parallel edges come from a destination's largest or smallest source, the sign is chosen so that they are its
    maximal in-edges).  PARALLEL edges tie without the edge term; they differ only in their ef rows, so with it one of them wins wherever
    qe . (ef_1 - ef_2) != 0.  ASSERTED here: at least one (destination, head) has such a pair (`split`); every logit's absolute terms stay
    below 2^24; the maximal in-edges of every (destination, head) share one source; the absolute terms of every compared sum stay below
    2^22.  Returns the operands (ef in POSITION order), out32 / aef32 (the float32 forward, bit for bit: c * float32(kept sum) /
    float32(count)), the float64 results and `single`."""
    src, dst = positions(g)
    n_src, n_dst, E = g.number_of_src_nodes(), g.number_of_dst_nodes(), src.numel()
    rng = np.random.default_rng(seed)
    if lim is None:
        lim = 8 if D <= 5 else max(1, min(8, int((1700.0 / (2 * (D - 1))) ** 0.5)))
    R = K * 2 * elim
    q, k = DC._ints(rng, -lim, lim, (n_dst, H, D)), DC._ints(rng, -lim, lim, (n_src, H, D))
    q[:, :, 0] = DC._ints(rng, 0, 1, (n_dst, H)) * 2 - 1
    pair, times = torch.unique(dst * n_src + src, return_counts=True)      # a destination whose largest (smallest) source sends parallel
    for e in pair[times > 1].tolist():                                     # edges looks up (down), so that those edges are its maximal ones
        vv, uu = divmod(e, n_src)
        mine = src[dst == vv]
        if uu == int(mine.max()) or uu == int(mine.min()):
            q[vv, :, 0] = 1.0 if uu == int(mine.max()) else -1.0
    k[:, :, 0] = (torch.arange(n_src, dtype=torch.float32) + 1).view(-1, 1) * (2 * (lim * lim * (D - 1) + R) + 1)
    v, dout = DC._ints(rng, -lim, lim, (n_src, H, D)), DC._ints(rng, -lim, lim, (n_dst, H, D))
    qe = (DC._ints(rng, 1, 2, (n_dst, H, K)) * (DC._ints(rng, 0, 1, (n_dst, H, K)) * 2 - 1))
    ef, daef = DC._ints(rng, -elim, elim, (E, K)), DC._ints(rng, -lim, lim, (n_dst, H, K))
    scale = 128.0
    q64, k64, v64, d64, qe64, ef64, dae64 = (t.double() for t in (q, k, v, dout, qe, ef, daef))
    assert float(((q64[dst] * k64[src]).abs().sum(-1) + (qe64[dst] * ef64.unsqueeze(1)).abs().sum(-1)).max()) < 2.0 ** 24
    fwd = forward64(src, dst, n_dst, q64, k64, v64, ef64, qe64, scale, keep, c)
    idx = dst.view(-1, 1).expand(-1, H)
    top_of = lambda s: s == torch.zeros((n_dst, H), dtype=F64).scatter_reduce(0, idx, s, "amax", include_self=False)[dst]
    top = top_of(fwd["s"])
    plain_top = top_of((q64[dst] * k64[src]).sum(-1) * scale)                # the maximal in-edges WITHOUT the edge term
    count, plain_count = _tot(n_dst, dst, top.double()), _tot(n_dst, dst, plain_top.double())
    split = (plain_count > 1) & (count < plain_count)
    assert int(split.sum()) > 0, "no parallel pair is separated by its edge features"
    srcs = src.view(-1, 1).expand(-1, H)
    lo = torch.full((n_dst, H), n_src, dtype=torch.int64).scatter_reduce(0, idx, torch.where(top, srcs, n_src), "amin", include_self=True)
    hi = torch.full((n_dst, H), -1, dtype=torch.int64).scatter_reduce(0, idx, torch.where(top, srcs, -1), "amax", include_self=True)
    assert bool((lo == hi)[fwd["deg"] > 0].all()), "two distinct sources tie for the largest logit of a (destination, head)"
    a = top.double() / count[dst].clamp(min=1)
    assert bool(((fwd["a"] - a).abs() < 1e-30).all())                      # the losers' weights are below exp(-128)
    fwd["a"] = a
    fwd["w"] = a if keep is None else a * keep.double() * c
    fwd["out"] = _tot(n_dst, dst, fwd["w"].unsqueeze(-1) * v64[src])
    fwd["aef"] = _tot(n_dst, dst, fwd["w"].unsqueeze(-1) * ef64.unsqueeze(1))
    kept = top.double() if keep is None else top.double() * keep.double()
    tot_v, tot_e = _tot(n_dst, dst, kept.unsqueeze(-1) * v64[src]), _tot(n_dst, dst, kept.unsqueeze(-1) * ef64.unsqueeze(1))
    assert float(_tot(n_dst, dst, kept.unsqueeze(-1) * v64[src].abs()).max()) < DC.EXACT_LIMIT
    cf, cnt = torch.tensor(c, dtype=torch.float32), count.clamp(min=1).float().unsqueeze(-1)
    out32, aef32 = cf * (tot_v.float() / cnt), cf * (tot_e.float() / cnt)     # c is 1 or 2 here: exact
    bwd = backward64(src, dst, n_src, n_dst, q64, k64, v64, ef64, qe64, scale, d64, dae64, fwd, keep, c)
    single = (count == 1) | (fwd["deg"] == 0).view(-1, 1)
    assert bool((bwd["ds"][single[dst]] == 0).all())                         # one maximal in-edge: dd = delta, so ds = 0
    return dict(q=q, k=k, v=v, dout=dout, qe=qe, ef=ef, daef=daef, scale=scale, out32=out32, aef32=aef32, fwd=fwd, bwd=bwd, src=src, dst=dst,
                single=single, split=split)


def onehot_backward_from_lse(case, lse32, D, K, c=1.0, keep=None):
    """`dot_attn_cases.onehot_backward_from_lse` with the edge term: the gradients the contract defines from the float32 lse the kernel
    returned and its float32 out and aef (bit for bit out32 / aef32), with the bounds of that argument: rho = 2 EXP_ERR + 2 U, out and
    aef given.  -> (bwd, bounds)."""
    src, dst = case["src"], case["dst"]
    q64, k64, v64, d64, qe64, ef64, dae64 = (case[n].double() for n in ("q", "k", "v", "dout", "qe", "ef", "daef"))
    n_src, n_dst = k64.shape[0], q64.shape[0]
    fwd = dict(case["fwd"])
    fwd["a"] = torch.exp(fwd["s"] - lse32.double()[dst])
    fwd["out"], fwd["aef"] = case["out32"].double(), case["aef32"].double()
    bwd = backward64(src, dst, n_src, n_dst, q64, k64, v64, ef64, qe64, case["scale"], d64, dae64, fwd, keep, c)
    bb = backward_bounds(src, dst, n_src, n_dst, q64, k64, v64, ef64, case["scale"], d64, dae64, fwd, bwd, None, D, K, c,
                         rho=2 * EXP_ERR + 2 * U, given=True)
    tiny = 1e-37
    return bwd, {n: t + tiny * (1 + abs(case["scale"]) * 2.0 ** 24) for n, t in bb.items()}


# ------------------------------------------------------------------------------------------------ shared checks of the layer and the stack
def check_layer(conv, g, dev, fin, ef, pair=False, seed=0):
    """`dot_attn_cases.check_layer` for a layer that takes edge_attr (edge-id order)."""
    ef_pos = ef[eid_of_positions(g)].double()
    ref64 = lambda c, src, dst, n_dst, xs, xd, p: edge_transformer_conv64(c, src, dst, n_dst, xs, xd, p, ef_pos)
    return DC.check_layer(_WithEdgeAttr(conv, ef.to(dev)), ref64, g, dev, fin, seed=seed, pair=pair)


class _WithEdgeAttr:
    """A layer with its edge_attr bound, for `dot_attn_cases.check_layer`, which calls `conv(g, feat)`: everything else is the layer's."""

    def __init__(self, conv, ef):
        self._conv, self._ef = conv, ef

    def __call__(self, graph, feat):
        return self._conv(graph, feat, self._ef)

    def to(self, dev):
        self._conv.to(dev)
        return self

    def __getattr__(self, name):
        return getattr(self._conv, name)


def check_stack(model, graphs, feat, dev, edge_feats=None):
    """`dot_attn_cases.check_stack` for `EdgeUniMP`: eval mode on a Graph or a block list against `edge_unimp_stack64`."""
    from tests.gatv2_cases import params64
    from tests.parity_cases import fwd_close, grad_close
    blocks = graphs if isinstance(graphs, (list, tuple)) else None
    per_layer = list(blocks) if blocks is not None else [graphs] * model.n_layers
    model = model.to(dev).eval()
    model.zero_grad(set_to_none=True)
    with torch.no_grad():
        gen = torch.Generator().manual_seed(11)
        for bn in model.norms:
            bn.running_mean.copy_(0.3 * torch.randn(bn.running_mean.shape, generator=gen))
            bn.running_var.copy_(0.5 + torch.rand(bn.running_var.shape, generator=gen))
    x = feat.detach().clone().to(dev).requires_grad_()
    out = model(graphs, x, edge_feats=edge_feats)
    dout = torch.randn(out.shape, generator=torch.Generator().manual_seed(12))
    out.backward(dout.to(dev))
    p = params64(model)
    f64 = feat.detach().cpu().double().requires_grad_()
    layers = []
    for i, g in enumerate(per_layer):
        ef = g.edata["feat"] if edge_feats is None else (edge_feats[i] if isinstance(edge_feats, (list, tuple)) else
                                                         (g.edata[edge_feats] if isinstance(edge_feats, str) else edge_feats))
        src, dst = positions(g)
        layers.append((src, dst, g.number_of_dst_nodes(), ef.cpu().double()[eid_of_positions(g)]))
    ref = edge_unimp_stack64(model, layers, f64, p)
    ref.backward(dout.double())
    fwd_close(out, ref.detach().numpy())
    grad_close(x.grad, f64.grad.numpy())
    DC.param_grads_close(model, p)
