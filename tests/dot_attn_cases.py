"""Float64 restatements of the dot-product attention contracts (include/bot_gnn.h "Dot-product attention"), shared by
tests/test_dot_attn_host.py and tests/test_dot_attn_gpu.py: the forward with lse, the three analytic gradients with the absolute sums
their rounding bounds are made of, `DotGatConv` / `TransformerConv` / `UniMP` as differentiable float64 torch, the input builders of the
exact regimes (with their conditions ASSERTED while the inputs are built) and the bound functions.  Nothing here calls the code under
test, except the `check_*` functions at the end, which run it against the restatements on whatever device the graph lives on."""
import numpy as np
import torch

from tests.gatv2_cases import EXACT_LIMIT, F64, U, degree_of, edge_lists, layer_params, params64, positions  # noqa: F401

EXP_ERR = 1.278e-07       # the measured relative error of smx_exp over [-87, 0] (README "DeeperGCN")


def _tot(n, idx, x):
    return torch.zeros((n,) + tuple(x.shape[1:]), dtype=F64).index_add_(0, idx, x)


# ------------------------------------------------------------------------------------------------ the op, float64
def attention64(src, dst, n_dst, q, k, v, scale, keep=None, c=1.0):
    """The forward as differentiable float64 torch: out [n_dst, H, D] = c sum_k keep_k a_k v[u_k], a = softmax over a destination's
    in-edges of scale * <q[v], k[u]>.  keep: bool [E, H] or None."""
    s = (q[dst] * k[src]).sum(-1) * scale                                  # [E, H]
    idx = dst.view(-1, 1).expand(-1, s.shape[1])
    m = torch.full((n_dst, s.shape[1]), -np.inf, dtype=s.dtype).scatter_reduce(0, idx, s.detach(), "amax", include_self=True)
    ex = torch.exp(s - m[dst])
    den = torch.zeros((n_dst, s.shape[1]), dtype=s.dtype).index_add(0, dst, ex)
    a = ex / den[dst]
    w = a if keep is None else a * keep.to(a.dtype) * c
    return torch.zeros((n_dst,) + tuple(v.shape[1:]), dtype=v.dtype).index_add(0, dst, w.unsqueeze(-1) * v[src])


def forward64(src, dst, n_dst, q, k, v, scale, keep=None, c=1.0):
    """The forward contract in float64 from float64 operands: a dict with out [n_dst, H, D], lse [n_dst, H] (0 on an empty row), the
    weights a [E, H], the logits s, and what the bounds are made of: deg, sabs = scale sum_d |q k| per edge, vmax = the largest |v| a
    (destination, column) gathers."""
    H = q.shape[1]
    s = (q[dst] * k[src]).sum(-1) * scale
    sabs = (q[dst] * k[src]).abs().sum(-1) * abs(scale)
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
    vidx = dst.view(-1, 1, 1).expand(-1, H, v.shape[2])
    vmax = torch.zeros((n_dst, H, v.shape[2]), dtype=F64).scatter_reduce(0, vidx, v[src].abs(), "amax", include_self=True)
    amax = lambda t: torch.zeros((n_dst, H), dtype=F64).scatter_reduce(0, idx, t, "amax", include_self=True)
    return dict(out=out, lse=lse, a=a, w=w, s=s, deg=deg, sabs=sabs, vmax=vmax, smax=amax(s.abs()), sabs_max=amax(sabs))


def backward64(src, dst, n_src, n_dst, q, k, v, scale, dout, fwd, keep=None, c=1.0):
    """The three analytic gradients of the contract in float64, and per-edge pieces the bounds need: a dict with dq, dk, dv, p, ds
    ([E, H]), ddabs = sum_d |dout v| per edge and delabs = sum_d |dout out| per destination."""
    a, out = fwd["a"], fwd["out"]
    ck = torch.full_like(a, 1.0) if keep is None else keep.to(F64) * c
    delta = (dout * out).sum(-1)                                           # [n_dst, H]
    dd = (dout[dst] * v[src]).sum(-1)
    p = ck * a
    ds = a * (ck * dd - delta[dst])
    dq = scale * _tot(n_dst, dst, ds.unsqueeze(-1) * k[src])
    dk = scale * _tot(n_src, src, ds.unsqueeze(-1) * q[dst])
    dv = _tot(n_src, src, p.unsqueeze(-1) * dout[dst])
    return dict(dq=dq, dk=dk, dv=dv, p=p, ds=ds, ck=ck, ddabs=(dout[dst] * v[src]).abs().sum(-1), delabs=(dout * out).abs().sum(-1))


def forward_bounds(fwd, D, c=1.0):
    """Per-entry bounds on |kernel - forward64| for out and lse, derived from the lengths (as tests/gen_cases.forward_bounds).  The
    kernel keeps Z and S as sequential sums in position order, one product and one fused multiply-add per term: two roundings per term,
    (2 deg + 3) U with the division and the factor c.  A term's weight is a product of at most deg exponentials (its own and every later
    rescale), in the numerator and in the denominator: 2 deg (2 EXP_ERR), EXP_ERR the measured relative error of smx_exp with a margin of
    2.  The logit itself is a rounded sum: (D + 3) U scale sum_d |q k| (D products, the sum, the scale), and the exponent's argument s - M
    two more roundings of at most U max|s| each, of s and of M: eps = (D + 3) U max_k sabs + 4 U max|s| is an ABSOLUTE error of every
    exponent of the row, so every weight moves by a relative 2 eps at most (numerator and denominator); out is a weighted mean of
    entries bounded by vmax, so it moves by at most 2 (2 eps) vmax.  lse = M + log Z: the relative error of Z, eps directly, the rounding
    of M, of the logarithm and of the sum, 4 U (max|s| + |lse|) + 2 U."""
    deg = fwd["deg"].view(-1, 1)
    eps = (D + 3) * U * fwd["sabs_max"] + 4 * U * fwd["smax"]
    rel = (2 * deg + 3) * U + 2 * deg * 2 * EXP_ERR
    return dict(out=(rel + 4 * eps).unsqueeze(-1) * c * fwd["vmax"], eps=eps, rel=rel,
                lse=deg * (2 * U + 4 * EXP_ERR) + 2 * eps + 4 * U * (fwd["smax"] + fwd["lse"].abs()) + 2 * U)


def backward_bounds(src, dst, n_src, n_dst, q, k, v, scale, dout, fwd, bwd, fb, D, c=1.0, rho=None, out_given=False):
    """Per-entry bounds for dq, dk, dv (and p, ds per edge), the same form with the row lengths.  The backward's weight a_k = exp(s_k -
    lse) carries rho = 2 EXP_ERR + eps (its logit) + the forward's lse bound + 2 U (max|s| + |lse|) (the argument's roundings), relative.
    ds_k = a_k (c keep dd_k - delta): dd and delta are rounded sums of D products, (D + 2) U of their absolute terms, delta also moves
    with out (sum_d |dout| out_bound); three more roundings for the products and the difference.  A gradient entry is a sequential sum
    of ds_k (or p_k) times an exact operand entry: the terms' own errors plus (row length + 3) U of the sum of their absolute values,
    the row length being the in-degree for dq and the out-degree for dk and dv.  `rho`: the weights' relative error where the caller
    knows it better (the one-hot regime, whose expectation is built from the float32 lse the kernel returned); `out_given`: fwd["out"]
    is the float32 out the kernel read, so delta does not move with it."""
    a, ck = fwd["a"], bwd["ck"]
    if rho is None:
        rho = (2 * EXP_ERR + fb["eps"] + fb["lse"] + 2 * U * (fwd["smax"] + fwd["lse"].abs()))[dst]             # [E, H]
    mag = ck * bwd["ddabs"] + bwd["delabs"][dst]                           # >= |c keep dd - delta| in absolute terms
    d_err = 0.0 if out_given else (dout.abs() * fb["out"]).sum(-1)[dst]
    ds_err = a * ((rho + (D + 5) * U) * mag + d_err)
    ds_abs = a * mag
    p_err = ck * a * (rho + 2 * U)
    s = abs(scale)
    deg_in, deg_out = degree_of(dst, n_dst).view(-1, 1, 1), degree_of(src, n_src).view(-1, 1, 1)
    e3 = lambda t: t.unsqueeze(-1)
    dq = s * (_tot(n_dst, dst, e3(ds_err) * k[src].abs()) + (deg_in + 4) * U * _tot(n_dst, dst, e3(ds_abs) * k[src].abs()))
    dk = s * (_tot(n_src, src, e3(ds_err) * q[dst].abs()) + (deg_out + 4) * U * _tot(n_src, src, e3(ds_abs) * q[dst].abs()))
    dv = _tot(n_src, src, e3(p_err) * dout[dst].abs()) + (deg_out + 3) * U * _tot(n_src, src, e3(bwd["p"]) * dout[dst].abs())
    return dict(dq=dq, dk=dk, dv=dv, p=p_err, ds=ds_err + 3 * U * ds_abs,
                dkv=dk + dv + U * (bwd["dk"].abs() + bwd["dv"].abs()))


# ------------------------------------------------------------------------------------------------ input builders
def normal_inputs(n_src, n_dst, H, D, seed):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(shape, generator=gen)
    return r(n_dst, H, D), r(n_src, H, D), r(n_src, H, D), r(n_dst, H, D)       # q, k, v, dout


def draw_keep(E, H, p, seed):
    return torch.rand((E, H), generator=torch.Generator().manual_seed(seed)) >= p


def _ints(rng, lo, hi, shape):
    return torch.from_numpy(rng.integers(lo, hi + 1, shape).astype(np.float32))


def uniform_inputs(g, H, D, seed, lim=8):
    """Exact regime A: q = 0, so every weight of a row is 1 / deg; integer-valued v and dout, k arbitrary integers.  Returns (q, k, v,
    dout) and the exact results: sum_v [n_dst, H, D] (float64 of a sum whose absolute terms are asserted below 2^22) and deg."""
    src, dst = positions(g)
    n_src, n_dst = g.number_of_src_nodes(), g.number_of_dst_nodes()
    rng = np.random.default_rng(seed)
    q = torch.zeros(n_dst, H, D)
    k, v, dout = _ints(rng, -lim, lim, (n_src, H, D)), _ints(rng, -lim, lim, (n_src, H, D)), _ints(rng, -lim, lim, (n_dst, H, D))
    assert float(_tot(n_dst, dst, v.double()[src].abs()).max()) < EXACT_LIMIT
    return (q, k, v, dout), src, dst


def onehot_inputs(g, H, D, seed, lim=None, shared=False, keep=None, c=1.0):
    """Exact regime B: integer-valued q, k in [-lim, lim] and scale = 128, so two logits of a row are equal or at least 128 apart and
    every weight is 0 or 1 / (number of maximal in-edges).  k[u, h, 0] = (u + 1) (2 lim^2 (D - 1) + 1) and q[v, h, 0] = +-1: two DISTINCT
    sources never tie, only parallel edges do, so the maximal in-edges of a (destination, head) all gather ONE v row and out is c *
    float32(kept copies * v) / float32(copies): a true division of two exact integers, bit for bit whatever the number of copies (the
    one-row graph has 12 parallel in-edges from its one source, so a power-of-two count cannot be had by choosing seeds).  lim=None:
    8, or for wide heads the largest range that keeps 12 copies of the separating component of 201 sources below 2^22 (D = 250: 1).
    Where a row has one maximal in-edge ds is exactly 0 (dd = delta there), so dq and dk are exact zeros in those entries.  ASSERTED
    here, on the CPU: every logit's absolute terms stay below 2^24 (it is an exact integer times 128), the maximal in-edges of every
    (destination, head) share one source, and the absolute terms of every compared sum stay below 2^22.  Returns a dict: the operands,
    scale, out32 (the float32 forward, bit for bit), the float64 results (out, lse, dq, dk, dv, p, ds) and `single`, the (destination,
    head) pairs with ONE maximal in-edge.  A seed that violates a condition fails here, loudly."""
    src, dst = positions(g)
    n_src, n_dst = g.number_of_src_nodes(), g.number_of_dst_nodes()
    rng = np.random.default_rng(seed)
    if lim is None:
        lim = 8 if D <= 5 else max(1, min(8, int((1700.0 / (2 * (D - 1))) ** 0.5)))
    q, k = _ints(rng, -lim, lim, (n_dst, H, D)), _ints(rng, -lim, lim, (n_src, H, D))
    q[:, :, 0] = _ints(rng, 0, 1, (n_dst, H)) * 2 - 1
    k[:, :, 0] = (torch.arange(n_src, dtype=torch.float32) + 1).view(-1, 1) * (2 * lim * lim * (D - 1) + 1)
    v = k if shared else _ints(rng, -lim, lim, (n_src, H, D))
    dout = _ints(rng, -lim, lim, (n_dst, H, D))
    scale = 128.0
    q64, k64, v64, d64 = q.double(), k.double(), v.double(), dout.double()
    assert float((q64[dst] * k64[src]).abs().sum(-1).max()) < 2.0 ** 24 if src.numel() else True
    fwd = forward64(src, dst, n_dst, q64, k64, v64, scale, keep, c)
    top = (fwd["s"] == torch.zeros((n_dst, H), dtype=F64).scatter_reduce(0, dst.view(-1, 1).expand(-1, H), fwd["s"], "amax", include_self=False)[dst])
    count = _tot(n_dst, dst, top.double())
    idx = dst.view(-1, 1).expand(-1, H)
    srcs = src.view(-1, 1).expand(-1, H)
    lo = torch.full((n_dst, H), n_src, dtype=torch.int64).scatter_reduce(0, idx, torch.where(top, srcs, n_src), "amin", include_self=True)
    hi = torch.full((n_dst, H), -1, dtype=torch.int64).scatter_reduce(0, idx, torch.where(top, srcs, -1), "amax", include_self=True)
    assert bool((lo == hi)[fwd["deg"] > 0].all()), "two distinct sources tie for the largest logit of a (destination, head)"
    a = top.double() / count[dst].clamp(min=1)
    assert bool(((fwd["a"] - a).abs() < 1e-30).all())                      # the losers' weights are below exp(-128)
    fwd["a"] = a
    fwd["w"] = a if keep is None else a * keep.double() * c
    fwd["out"] = _tot(n_dst, dst, fwd["w"].unsqueeze(-1) * v64[src])
    kept = top.double() if keep is None else top.double() * keep.double()
    tot = _tot(n_dst, dst, kept.unsqueeze(-1) * v64[src])
    assert float(_tot(n_dst, dst, kept.unsqueeze(-1) * v64[src].abs()).max()) < EXACT_LIMIT if src.numel() else True
    out32 = torch.tensor(c, dtype=torch.float32) * (tot.float() / count.clamp(min=1).float().unsqueeze(-1))      # c is 1 or 2 here: exact
    bwd = backward64(src, dst, n_src, n_dst, q64, k64, v64, scale, d64, fwd, keep, c)
    single = (count == 1) | (fwd["deg"] == 0).view(-1, 1)
    assert bool((bwd["ds"][single[dst]] == 0).all())                         # one maximal in-edge: dd = delta, so ds = 0 and dq, dk are exact zeros
    t = _tot(n_src, src, (bwd["p"] * single[dst]).unsqueeze(-1) * d64[dst].abs())
    assert t.numel() == 0 or float(t.max()) < EXACT_LIMIT, float(t.max())
    return dict(q=q, k=k, v=v, dout=dout, scale=scale, out32=out32, fwd=fwd, bwd=bwd, src=src, dst=dst, single=single)


def onehot_backward_from_lse(case, lse32, D, c=1.0, keep=None):
    """The one-hot regime's gradients as the kernel's own contract gives them, in float64: the backward's weight is a_k = exp(s_k -
    lse[v, h]) of the float32 lse the forward left (`lse32`, held to 3 U |lse| by the caller) and delta is formed from the float32 out
    (bit for bit case["out32"]).  In this regime s_k is an exact float32 (an integer below 2^24 times 128) and s_k - lse is exact for
    every edge whose weight is not flushed to 0 (the two are within a factor of 2: Sterbenz), so a_k carries only smx_exp's measured
    error, 2 EXP_ERR with its margin; c keep dd is exact, delta is a rounded sum of D products, and the rest is the roundings of the
    products and of the sequential sums: `backward_bounds` with rho = 2 EXP_ERR + 2 U and the out given.  Relative to the sums' absolute
    terms these bounds are a few 1e-7 per term whatever the size of the logits, also where parallel edges tie.  -> (bwd, bounds)."""
    src, dst = case["src"], case["dst"]
    q64, k64, v64, d64 = (case[n].double() for n in ("q", "k", "v", "dout"))
    n_src, n_dst = k64.shape[0], q64.shape[0]
    fwd = dict(case["fwd"])
    fwd["a"] = torch.exp(fwd["s"] - lse32.double()[dst])
    fwd["out"] = case["out32"].double()
    bwd = backward64(src, dst, n_src, n_dst, q64, k64, v64, case["scale"], d64, fwd, keep, c)
    bb = backward_bounds(src, dst, n_src, n_dst, q64, k64, v64, case["scale"], d64, fwd, bwd, None, D, c, rho=2 * EXP_ERR + 2 * U, out_given=True)
    tiny = 1e-37                                                        # a flushed weight: below 2^-126 of a row total that is at least 1
    return bwd, {n: t + tiny * (1 + abs(case["scale"]) * 2.0 ** 24) for n, t in bb.items()}


def exact_entries(case, n_src):
    """Which gradient entries of a regime-B case are exact sums: the backward's weight exp(s - lse) is exactly 1 where the row has ONE
    maximal in-edge (lse = s there), while for m of them lse = s + log m is rounded at the size of s and exp(s - lse) is 1 / m only to
    within that rounding.  -> (dq_rows [n_dst, H], src_rows [n_src, H]): dq[v, h] where (v, h) is single, dk / dv[u, h] where every
    destination that u reaches is."""
    single = case["single"]
    bad = torch.zeros((n_src, single.shape[1]), dtype=F64).index_add_(0, case["src"], (~single[case["dst"]]).double())
    return single, bad == 0


# ------------------------------------------------------------------------------------------------ layers and stack, float64 torch
def _lin(x, p, name):
    y = x @ p[name + ".weight"].t()
    b = p.get(name + ".bias")
    return y if b is None else y + b


def dotgat_conv64(conv, src, dst, n_dst, h_src, h_dst, p):
    H, D = conv._num_heads, conv._out_feats
    kv = (h_src @ p["fc.weight"].t()).view(-1, H, D)
    q = (h_dst @ p["fc.weight"].t()).view(-1, H, D)
    return attention64(src, dst, n_dst, q, kv, kv, D ** -0.5)


def transformer_conv64(conv, src, dst, n_dst, x_src, x_dst, p, keep=None):
    """`TransformerConv` in float64; keep: the drawn attention-dropout mask (bool [E, H], CSC position order - then src / dst must be
    the CSC positions) or None for drop rate 0."""
    H, C = conv.heads, conv.out_channels
    q, k, v = (_lin(x, p, n).view(-1, H, C) for x, n in ((x_dst, "lin_query"), (x_src, "lin_key"), (x_src, "lin_value")))
    out = attention64(src, dst, n_dst, q, k, v, C ** -0.5, keep, 1.0 if keep is None else 1.0 / (1.0 - conv.dropout))
    out = out.reshape(-1, H * C) if conv.concat else out.mean(1)
    if conv.root_weight:
        x_r = _lin(x_dst, p, "lin_skip")
        if conv.lin_beta is not None:
            b = torch.sigmoid(torch.cat([out, x_r, out - x_r], dim=-1) @ p["lin_beta.weight"].t())
            out = b * x_r + (1 - b) * out
        else:
            out = out + x_r
    return out


def unimp_stack64(model, layers, feat, p):
    """`UniMP` in eval mode (no dropout, BatchNorm by its running statistics) in float64; layers: per layer (src, dst, n_dst)."""
    h = feat
    n = len(model.convs)
    for i, (src, dst, n_dst) in enumerate(layers):
        h = transformer_conv64(model.convs[i], src, dst, n_dst, h, h[:n_dst], layer_params(p, i))
        if i < n - 1:
            if len(model.norms):
                bn = model.norms[i]
                h = (h - bn.running_mean.cpu().double()) * torch.rsqrt(bn.running_var.cpu().double() + bn.eps) * p[f"norms.{i}.weight"] + p[f"norms.{i}.bias"]
            h = torch.relu(h)
    return h


# ------------------------------------------------------------------------------------------------ shared checks
def check_op(g, dev, H, D, seed, impl=None, shared=False, p=0.0, worst=None, scale=None):
    """`ops.dot_attention` forward and the three gradients on seeded normal inputs against float64 under the derived bounds; returns the
    device results and the bounds (dicts keyed out / dq / dk / dv, or dkv when shared).  p > 0: a drawn keep mask.  `worst`: a dict that
    collects the largest error as a fraction of its bound."""
    from bot_amd import ops
    src, dst = positions(g)
    n_src, n_dst, E = g.number_of_src_nodes(), g.number_of_dst_nodes(), src.numel()
    q, k, v, dout = normal_inputs(n_src, n_dst, H, D, seed)
    if shared:
        v = k
    keep = draw_keep(E, H, p, seed + 1) if p > 0 else None
    c = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    sc = D ** -0.5 if scale is None else scale
    q64, k64, v64, d64 = q.double(), k.double(), v.double(), dout.double()
    fwd = forward64(src, dst, n_dst, q64, k64, v64, sc, keep, c)
    bwd = backward64(src, dst, n_src, n_dst, q64, k64, v64, sc, d64, fwd, keep, c)
    fb = forward_bounds(fwd, D, c)
    bb = backward_bounds(src, dst, n_src, n_dst, q64, k64, v64, sc, d64, fwd, bwd, fb, D, c)
    ql, kl = q.clone().to(dev).requires_grad_(), k.clone().to(dev).requires_grad_()
    vl = kl if shared else v.clone().to(dev).requires_grad_()
    out = ops.dot_attention(g, ql, kl, vl, scale, keep=None if keep is None else keep.to(dev), p=p, impl=impl)
    assert out.shape == (n_dst, H, D) and out.dtype == torch.float32
    out.backward(dout.to(dev))
    got = dict(out=out.detach(), dq=ql.grad)
    want, lim = dict(out=fwd["out"], dq=bwd["dq"]), dict(out=fb["out"], dq=bb["dq"])
    if shared:
        got["dkv"], want["dkv"], lim["dkv"] = kl.grad, bwd["dk"] + bwd["dv"], bb["dkv"]
    else:
        got.update(dk=kl.grad, dv=vl.grad), want.update(dk=bwd["dk"], dv=bwd["dv"]), lim.update(dk=bb["dk"], dv=bb["dv"])
    got = {n: t.cpu().double() for n, t in got.items()}
    for name in got:
        err = (got[name] - want[name]).abs()
        frac = float((err / lim[name].clamp(min=1e-300)).max()) if err.numel() else 0.0
        if worst is not None:
            worst[name] = max(worst.get(name, 0.0), frac)
        assert bool((err <= lim[name]).all()), (name, H, D, impl, frac)
    return got, lim


def seeded(module, seed):
    """Seeded non-zero biases (torch initialises some to values that hide a dropped bias)."""
    gen = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for name, prm in module.named_parameters():
            if name.endswith("bias"):
                prm.copy_(torch.randn(prm.shape, generator=gen))
    return module


def param_grads_close(module, p):
    """Every parameter's gradient against the float64 one under tests/parity_cases.grad_close.  One exception, with its reason: the
    key bias shifts every logit of a destination by the same q[v] . b, which the softmax ignores, so its gradient is analytically ZERO
    and what either side holds is the cancellation noise of a sum over all edges.  A bias is a weight column on a constant-1 input, so
    it is held to the absolute tolerance of its own weight matrix: GRAD_RTOL times the largest entry of lin_key.weight's gradient."""
    from tests.parity_cases import GRAD_RTOL, grad_close
    for name, prm in module.named_parameters():
        if name.endswith("lin_key.bias"):
            scale = float(p[name[:-4] + "weight"].grad.abs().max())
            err = float((prm.grad.detach().cpu().double() - p[name].grad).abs().max())
            assert err <= GRAD_RTOL * scale, (name, err, scale)
        else:
            grad_close(prm.grad, p[name].grad.numpy())


def check_layer(conv, ref64, g, dev, fin, seed=0, pair=False, keep=None):
    """One layer forward + backward on `g` against its float64 restatement `ref64(conv, src, dst, n_dst, x_src, x_dst, p)` under the
    suite's own criteria (tests/parity_cases.py): the output and the gradients of the input(s) and of every parameter."""
    from tests.parity_cases import fwd_close, grad_close
    src, dst = positions(g)                                 # CSC position order: what a drawn keep mask is indexed by
    n_src, n_dst = g.number_of_src_nodes(), g.number_of_dst_nodes()
    conv = conv.to(dev)
    gen = torch.Generator().manual_seed(seed + 1)
    x_src = torch.randn(n_src, fin, generator=gen)
    x_dst = torch.randn(n_dst, fin, generator=gen) if pair else None
    xs = x_src.clone().to(dev).requires_grad_()
    xd = None if x_dst is None else x_dst.clone().to(dev).requires_grad_()
    out = conv(g, (xs, xd) if pair else xs)
    dout = torch.randn(out.shape, generator=gen)
    out.backward(dout.to(dev))
    p = params64(conv)
    s64 = x_src.double().requires_grad_()
    d64 = None if x_dst is None else x_dst.double().requires_grad_()
    kw = {} if keep is None else dict(keep=keep)
    ref = ref64(conv, src, dst, n_dst, s64, s64[:n_dst] if d64 is None else d64, p, **kw)
    assert tuple(out.shape) == tuple(ref.shape)
    ref.backward(dout.double())
    fwd_close(out, ref.detach().numpy())
    grad_close(xs.grad, s64.grad.numpy())
    if pair:
        grad_close(xd.grad, d64.grad.numpy())
    param_grads_close(conv, p)
    return conv


def check_stack(model, graphs, feat, dev):
    """`UniMP` in eval mode on a Graph or a block list against `unimp_stack64`: output, input gradient, every parameter's gradient."""
    from tests.parity_cases import fwd_close, grad_close
    blocks = graphs if isinstance(graphs, (list, tuple)) else None
    per_layer = list(blocks) if blocks is not None else [graphs] * model.n_layers
    model = model.to(dev).eval()
    model.zero_grad(set_to_none=True)
    with torch.no_grad():
        gen = torch.Generator().manual_seed(11)
        for bn in model.norms:                         # running statistics that do something
            bn.running_mean.copy_(0.3 * torch.randn(bn.running_mean.shape, generator=gen))
            bn.running_var.copy_(0.5 + torch.rand(bn.running_var.shape, generator=gen))
    x = feat.detach().clone().to(dev).requires_grad_()
    out = model(graphs, x)
    dout = torch.randn(out.shape, generator=torch.Generator().manual_seed(12))
    out.backward(dout.to(dev))
    p = params64(model)
    f64 = feat.detach().cpu().double().requires_grad_()
    layers = [edge_lists(g)[:2] + (g.number_of_dst_nodes(),) for g in per_layer]
    ref = unimp_stack64(model, layers, f64, p)
    ref.backward(dout.double())
    fwd_close(out, ref.detach().numpy())
    grad_close(x.grad, f64.grad.numpy())
    param_grads_close(model, p)
