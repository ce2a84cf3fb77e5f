"""Numpy / float64 restatements of the softmax-aggregation contracts (include/bot_gnn.h "Softmax aggregation"), shared by
tests/test_gen_host.py and tests/test_gen_gpu.py: the forward with its row statistics, dx over the out-edges, dbeta, the error bounds
the GPU suite holds the kernels to, a float32 restatement of the two exact regimes, and float64 torch restatements of `GENConv` and
`DeeperGCN` with the `check_*` functions both suites share.  The restatements call nothing of the code under test.  Graphs come from
tests.sage_cases (`small_graph`, `csc_of`) and tests.test_subgraph_gpu (`_hub_graph`)."""
import numpy as np
import torch

from tests.sage_cases import csc_of, edge_lists, params64, small_graph  # noqa: F401 - re-exported for the two suites

F64 = torch.float64
U = 2.0 ** -24            # unit roundoff of float32
TINY = 2.0 ** -126        # the smallest normal float32: what a flushed exponential is off by at most


def message64(x, relu, eps):
    x = np.asarray(x, dtype=np.float64)
    return np.maximum(x, 0.0) + eps if relu else x


def _positions(indptr, rows):
    """(pos, seg, deg): the CSC positions of `rows` one after the other, the index into `rows` of each, and the rows' lengths."""
    deg = (indptr[rows + 1] - indptr[rows]).astype(np.int64)
    seg = np.repeat(np.arange(len(rows)), deg)
    first = np.repeat(indptr[rows].astype(np.int64) - np.concatenate([[0], np.cumsum(deg)[:-1]]), deg)
    return first + np.arange(int(deg.sum())), seg, deg


def forward64(indptr, indices, x, beta, relu=False, eps=0.0, rows=None):
    """The contract in float64 for the destination rows `rows` (default: all): dict of out, lse, q [len(rows), F] (zeros on an empty
    row), deg [len(rows)] and mabs [len(rows), F], the largest |m| of each (row, column)."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    rows = np.arange(len(indptr) - 1) if rows is None else np.asarray(rows, dtype=np.int64)
    pos, seg, deg = _positions(indptr, rows)
    F = x.shape[1]
    res = {k: np.zeros((len(rows), F)) for k in ("out", "lse", "q", "mabs")}
    res["deg"] = deg
    if pos.size == 0:
        return res
    m = message64(x, relu, eps)[indices[pos]]
    b = float(beta) * m
    some = deg > 0
    starts = (np.cumsum(deg) - deg)[some]
    mx = np.maximum.reduceat(b, starts, axis=0)
    e = np.exp(b - np.repeat(mx, deg[some], axis=0))
    Z = np.add.reduceat(e, starts, axis=0)
    res["out"][some] = np.add.reduceat(e * m, starts, axis=0) / Z
    res["q"][some] = np.add.reduceat(e * m * m, starts, axis=0) / Z
    res["lse"][some] = mx + np.log(Z)
    res["mabs"][some] = np.maximum.reduceat(np.abs(m), starts, axis=0)
    return res


def forward_bounds(res, beta, exp_err):
    """Per-entry bounds on |kernel - forward64| for out, lse and q.  The kernel keeps Z, S, Q as sequential sums in position order: one
    product and one fused multiply-add per term, so two roundings per term - (2 deg + 2) U with the division - times the row's largest
    |m| (Higham, Accuracy and Stability of Numerical Algorithms, section 3.1, as tests/test_smooth_gpu.py).  The exponential adds one
    term: exp_err, the measured relative error of the kernel's exponential, with a margin of 2 for arguments not sampled, per factor of
    a weight; a term's weight is a product of at most deg such factors (its own and every later rescale), in the numerator and in the
    denominator: 2 deg (2 exp_err).  out and q are weighted MEANS: the roundings of the exponential's argument beta m - M shift a weight
    a_k by a relative delta_k that enters only through a_k (m_k - out), and they get no term of their own here.  A flushed factor is
    off by at most 2^-126 of a row total that is at least 1: nothing beside U.  lse = M + log Z is not a mean: there the argument's
    roundings enter directly - of m (relu + eps), of the product beta m (in the entry and in M) and of the difference, at most 6 U B per
    factor with B = |beta| max|m| - beside the relative error of Z, the rounding of M (U B), of the logarithm (2 U |log Z| <= 2 U (|lse| +
    B)) and of the sum."""
    deg = res["deg"].astype(np.float64)[:, None]
    B = abs(float(beta)) * res["mabs"]
    rel = (2.0 * deg + 2.0) * U + 2.0 * deg * 2.0 * exp_err
    return {"out": rel * res["mabs"], "q": (rel + 2.0 * U) * res["mabs"] ** 2,
            "lse": deg * (2.0 * U + 2.0 * exp_err + 6.0 * U * B) + 4.0 * U * (B + np.abs(res["lse"])) + 2.0 * U}


def backward64(csr_indptr, csr_indices, x, beta, relu, eps, dout, out, lse, exp_err, rows=None):
    """(dx, bound) of the backward contract in float64 for the source rows `rows` (default: all), from the float32 operands the kernel
    gets: dx[u,f] = gate sum_j dout[v_j,f] exp(beta m_u - lse[v_j,f]) (1 + beta (m_u - out[v_j,f])).  Bound per entry: every term is
    d a c; a = exp(t) carries 2 exp_err + 4 U (|beta m_u| + |lse|) (the roundings of m_u, beta m_u and the difference) and TINY absolute;
    c = 1 + beta (m_u - out) four roundings of its parts; the products and the sequential sum (deg + 4) U of the term."""
    indptr, indices = np.asarray(csr_indptr, dtype=np.int64), np.asarray(csr_indices, dtype=np.int64)
    rows = np.arange(len(indptr) - 1) if rows is None else np.asarray(rows, dtype=np.int64)
    pos, seg, deg = _positions(indptr, rows)
    F = x.shape[1]
    dx, tol = np.zeros((len(rows), F)), np.zeros((len(rows), F))
    if pos.size == 0:
        return dx, tol
    beta = float(beta)
    xs = np.asarray(x, dtype=np.float64)[rows]
    m = message64(xs, relu, eps)[seg]
    v = indices[pos]
    d, o, l = (np.asarray(t, dtype=np.float64)[v] for t in (dout, out, lse))
    t = beta * m - l
    a = np.exp(t)
    c = 1.0 + beta * (m - o)
    term_tol = np.abs(d) * ((a * ((np.repeat(deg, deg)[:, None] + 4.0) * U + 2.0 * exp_err + 4.0 * U * (np.abs(beta * m) + np.abs(l))) + TINY) * np.abs(c)
                            + a * 4.0 * U * (1.0 + abs(beta) * (np.abs(m) + np.abs(o))))
    np.add.at(dx, seg, d * a * c)
    np.add.at(tol, seg, term_tol)
    gate = (xs > 0) if relu else np.ones_like(xs, dtype=bool)
    return np.where(gate, dx, 0.0), np.where(gate, tol, 0.0)


def dbeta64(res, dout):
    """dbeta = sum over (v, f) of dout (q - out^2), float64."""
    return float((np.asarray(dout, dtype=np.float64) * (res["q"] - res["out"] ** 2)).sum())


def dbeta_bound(res, tol, dout):
    """The op forms q - out^2 per entry in float32 (three roundings of q and out^2), multiplies by dout (one) and accumulates in float64;
    q and out carry the forward bounds; the result is rounded to float32 once."""
    d = np.abs(np.asarray(dout, dtype=np.float64))
    entry = tol["q"] + 2.0 * np.abs(res["out"]) * tol["out"] + tol["out"] ** 2 + 4.0 * U * (np.abs(res["q"]) + res["out"] ** 2)
    return float((d * entry).sum()) + U * abs(dbeta64(res, dout))


# ------------------------------------------------------------------------------------------------ the exact regimes, float32
def mean32(indptr, indices, x, relu):
    """beta = 0, eps = 0, integer-valued x: every weight is exactly 1, so out = float32(sum of m) / float32(deg); 0 on an empty row."""
    indptr = np.asarray(indptr, dtype=np.int64)
    deg = np.diff(indptr)
    m = np.asarray(x, dtype=np.float32)
    m = (np.maximum(m, 0) if relu else m)[np.asarray(indices, dtype=np.int64)].astype(np.int64)       # integer sums: exact in any order
    out = np.zeros((len(deg), x.shape[1]), dtype=np.float32)
    some = deg > 0
    if m.size:
        s = np.add.reduceat(m, indptr[:-1][some], axis=0).astype(np.float32)
        out[some] = s / deg[some].astype(np.float32)[:, None]
    return out


def max_backward64(csc_indptr, csc_indices, n_src, x, relu, dout):
    """beta = 128 with a unique maximum per (row, column): the whole gradient of a destination goes to the source that attains the max,
    gated by x > 0 under relu."""
    indptr, indices = np.asarray(csc_indptr, dtype=np.int64), np.asarray(csc_indices, dtype=np.int64)
    dx = np.zeros((n_src, x.shape[1]))
    cols = np.arange(x.shape[1])
    for r in range(len(indptr) - 1):
        b, e = indptr[r], indptr[r + 1]
        if e > b:
            u = indices[b:e][np.argmax(x[indices[b:e]], axis=0)]
            np.add.at(dx, (u, cols), np.asarray(dout[r], dtype=np.float64))
    return np.where(x > 0, dx, 0.0) if relu else dx


def simple_graph(n_dst, n_src, seed, chunk=None):
    """`small_graph` without parallel edges: every destination's sources are distinct (the same degree profile)."""
    import bot_amd
    rng = np.random.default_rng(seed)
    deg = rng.integers(1, 12, n_dst)
    deg[np.arange(n_dst) % 5 == 2] = 0
    if n_dst > 3:
        deg[3] = min(40, n_src)
    deg = np.minimum(deg, n_src)
    dst = np.repeat(np.arange(n_dst), deg)
    src = np.concatenate([rng.permutation(n_src)[:k] for k in deg]) if dst.size else np.zeros(0, dtype=np.int64)
    order = rng.permutation(dst.size)
    return bot_amd.Graph(torch.from_numpy(src[order]), torch.from_numpy(dst[order]), n_src, num_dst_nodes=n_dst, chunk=chunk)


# ------------------------------------------------------------------------------------------------ the layers, float64 torch
def softmax_agg64(src, dst, n_dst, msg, beta):
    """sum over the in-edges of softmax(beta msg) msg per destination and column: msg [E, F] in the order of src / dst; differentiable."""
    idx = dst.reshape(-1, 1).expand(-1, msg.shape[1])
    b = msg * beta
    mx = torch.full((n_dst, msg.shape[1]), -np.inf, dtype=msg.dtype).scatter_reduce(0, idx, b.detach(), "amax")
    e = torch.exp(b - mx[dst])
    zeros = torch.zeros((n_dst, msg.shape[1]), dtype=msg.dtype)
    Z = zeros.index_add(0, dst, e)
    return zeros.index_add(0, dst, e * msg) / torch.where(Z > 0, Z, torch.ones_like(Z))


def _bn_eval(h, bn, p, key):
    return (h - bn.running_mean.cpu().double()) * torch.rsqrt(bn.running_var.cpu().double() + bn.eps) * p[key + ".weight"] + p[key + ".bias"]


def _spread(scalar, shape, terms, key):
    """A one-element parameter as a tensor of `shape` whose gradient holds the TERMS of the parameter's gradient (kept in terms[key])."""
    t = scalar.reshape(()).expand(shape) * 1.0
    if terms is not None and t.requires_grad:
        t.retain_grad()
        terms[key] = t
    return t


def gen_conv64(conv, src, dst, n_dst, h_src, h_dst, p, ef=None, terms=None, prefix=""):
    """`GENConv` in eval mode in float64; p: the layer's named parameters as float64 tensors; ef: per-edge features in the order of src /
    dst; terms: a dict that receives, per one-element parameter (beta, msg_scale), the tensor whose .grad holds the terms of its gradient."""
    msg = torch.relu(h_src[src] if ef is None else h_src[src] + ef) + conv.eps
    beta = _spread(p["beta"], msg.shape, terms, prefix + "beta") if "beta" in p else conv.beta
    agg = softmax_agg64(src, dst, n_dst, msg, beta)
    if "msg_scale" in p:
        agg = torch.nn.functional.normalize(agg, p=2, dim=-1) * h_dst.norm(p=2, dim=-1, keepdim=True)
        agg = agg * _spread(p["msg_scale"], agg.shape, terms, prefix + "msg_scale")
    h = h_dst + agg
    for i in range(len(conv.mlp)):
        h = h @ p[f"mlp.{i}.weight"].t() + p[f"mlp.{i}.bias"]
        if i < len(conv.mlp) - 1:
            norm = conv.mlp_norms[i]
            if isinstance(norm, torch.nn.BatchNorm1d):
                h = _bn_eval(h, norm, p, f"mlp_norms.{i}")
            elif isinstance(norm, torch.nn.LayerNorm):
                h = torch.nn.functional.layer_norm(h, (h.shape[1],), p[f"mlp_norms.{i}.weight"], p[f"mlp_norms.{i}.bias"], norm.eps)
            h = torch.relu(h)
    return h


def _sub(p, prefix):
    return {k[len(prefix):]: v for k, v in p.items() if k.startswith(prefix)}


def deeper_gcn64(model, layers, feat, p, terms=None):
    """`DeeperGCN` in eval mode in float64; layers: per layer (src, dst, n_dst); terms: as in `gen_conv64`, keyed by parameter name."""
    h = feat @ p["node_encoder.weight"].t() + p["node_encoder.bias"]
    for i, (src, dst, n_dst) in enumerate(layers):
        cp = _sub(p, f"convs.{i}.")
        if i == 0:
            h = gen_conv64(model.convs[0], src, dst, n_dst, h, h[:n_dst], cp, None, terms, "convs.0.")
            continue
        t = torch.relu(_bn_eval(h, model.norms[i - 1], p, f"norms.{i - 1}"))
        h = gen_conv64(model.convs[i], src, dst, n_dst, t, t[:n_dst], cp, None, terms, f"convs.{i}.") + h[:n_dst]
    L = len(layers)
    h = torch.relu(_bn_eval(h, model.norms[L - 1], p, f"norms.{L - 1}"))
    return h @ p["output.weight"].t() + p["output.bias"]


def _stir(module, seed):
    """Biases and running statistics that do something."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, prm in module.named_parameters():
            if name.endswith("bias"):
                prm.copy_(0.3 * torch.randn(prm.shape, generator=gen))
        for mod in module.modules():
            if isinstance(mod, torch.nn.BatchNorm1d):
                mod.running_mean.copy_(0.3 * torch.randn(mod.running_mean.shape, generator=gen))
                mod.running_var.copy_(0.5 + torch.rand(mod.running_var.shape, generator=gen))


TERM_ERR = 1e-6           # relative error granted to one float32 TERM of a one-element gradient: a handful of roundings of 2^-24 each and
                          # an upstream gradient that is float32 itself; GRAD_RTOL / 100


def _compare(module, out, ref, p, x, x64, terms, extra=()):
    """The suite's criteria (tests/parity_cases.py): the output within FWD_ATOL, every gradient entry within GRAD_RTOL of the reference
    gradient's largest entry.  A ONE-ELEMENT gradient (beta, msg_scale) is held to the same criterion, GRAD_RTOL of its reference value,
    wherever a float32 computation can meet it.  It is a sum of signed terms and may cancel to any size; with every term good to TERM_ERR
    the sum is good to TERM_ERR times the terms' absolute sum, so the tolerance is max(GRAD_RTOL |ref|, TERM_ERR sum|t|): grad_close's
    own while the absolute sum is below 100 |ref|, and beyond that what the number format can give (the float32 tensor form on the CPU
    misses GRAD_RTOL |ref| on such a gradient: 4.2e-4 of a value of 4e-4).  README "DeeperGCN" states this deviation."""
    from tests.parity_cases import GRAD_RTOL, fwd_close, grad_close
    fwd_close(out, ref.detach().numpy())
    grad_close(x.grad, x64.grad.numpy())
    for name, prm in module.named_parameters():
        if not prm.requires_grad:
            continue
        if prm.numel() == 1:
            want, mass = float(p[name].grad), float(terms[name].grad.abs().sum())
            tol = max(GRAD_RTOL * abs(want), TERM_ERR * mass)
            assert abs(float(prm.grad) - want) <= tol, (name, float(prm.grad), want, mass)
        else:
            grad_close(prm.grad, p[name].grad.numpy())
    for got, want in extra:
        grad_close(got.grad, want.grad.numpy())


def check_conv(g, dev, fin, fout, seed=0, edge_feats=False, **kw):
    """One `GENConv` forward + backward in eval mode on `g` against `gen_conv64` under the suite's own criteria (tests/parity_cases.py):
    the output and the gradients of the input, of every trained parameter (beta and msg_scale included) and of the edge features."""
    from bot_amd import nn as bnn
    src, dst, n_src, n_dst, _ = edge_lists(g)
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    conv = bnn.GENConv(fin, fout, **kw)
    _stir(conv, seed + 1)
    conv = conv.to(dev).eval()
    feat = torch.randn(n_src, fin, generator=gen).to(dev).requires_grad_()
    dout = torch.randn(n_dst, fout, generator=gen)
    ef = torch.randn(src.numel(), fin, generator=gen) if edge_feats else None
    efl = None if ef is None else ef.clone().to(dev).requires_grad_()
    out = conv(g, feat, edge_feats=efl)
    out.backward(dout.to(dev))
    p = params64(conv)
    f64 = feat.detach().cpu().double().requires_grad_()
    e64 = None if ef is None else ef.double().requires_grad_()
    terms = {}
    ref = gen_conv64(conv, src, dst, n_dst, f64, f64[:n_dst], p, e64, terms)
    ref.backward(dout.double())
    assert out.shape == (n_dst, fout)
    _compare(conv, out, ref, p, feat, f64, terms, [] if ef is None else [(efl, e64)])
    return conv


def check_stack(model, graphs, feat, dev, seed=11):
    """`DeeperGCN` in eval mode on a Graph or a block list against `deeper_gcn64`: output, input gradient, every parameter's gradient."""
    blocks = graphs if isinstance(graphs, (list, tuple)) else None
    per_layer = list(blocks) if blocks is not None else [graphs] * model.n_layers
    _stir(model, seed)
    model = model.to(dev).eval()
    model.zero_grad(set_to_none=True)
    x = feat.detach().clone().to(dev).requires_grad_()
    out = model(graphs, x)
    dout = torch.randn(out.shape, generator=torch.Generator().manual_seed(seed + 1))
    out.backward(dout.to(dev))
    p = params64(model)
    f64 = feat.detach().cpu().double().requires_grad_()
    layers = []
    for g in per_layer:
        src, dst, _, n_dst, _ = edge_lists(g)
        layers.append((src, dst, n_dst))
    terms = {}
    ref = deeper_gcn64(model, layers, f64, p, terms)
    ref.backward(dout.double())
    _compare(model, out, ref, p, x, f64, terms)
