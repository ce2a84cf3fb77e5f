"""Float64 restatements of the GATv2 contracts (include/bot_gnn.h "GATv2 edge logits"), shared by tests/test_gatv2_host.py
and tests/test_gatv2_gpu.py: the edge logits with their three analytic gradients and the absolute sums the rounding bounds are made
of, the `GATv2Conv` layer and the `GATv2` stack as differentiable float64 torch; and the `check_*` functions that run the op, a layer
or a stack against them on whatever device the graph lives on.  The restatements call nothing of the code under test."""
import numpy as np
import torch

F64 = torch.float64
U = 2.0 ** -24            # the unit roundoff of float32
EXACT_LIMIT = 2.0 ** 22   # sums of multiples of 0.25 whose absolute terms add up to less than this are exact in float32


# ------------------------------------------------------------------------------------------------ the op
def positions(g):
    """(src, dst) of every CSC position of a graph, int64 CPU tensors."""
    indptr, indices = g.csc.indptr.cpu().long(), g.csc.indices.cpu().long()
    n = indptr.numel() - 1
    return indices, torch.repeat_interleave(torch.arange(n), indptr[1:] - indptr[:-1])


def _lrelu(s, slope):
    return torch.where(s > 0, s, slope * s)


def logits_forward(src, dst, fs, fd, attn, slope):
    """(e [E, H], sum_d |attn * lrelu(s)| [E, H]) in float64; fs [n_src, H, D], fd [n_dst, H, D], attn [H, D] as float64 tensors."""
    terms = attn.unsqueeze(0) * _lrelu(fs[src] + fd[dst], slope)
    return terms.sum(-1), terms.abs().sum(-1)


def logits_backward(src, dst, fs, fd, attn, slope, de):
    """The analytic gradients of the contract and, for each, the sum of the absolute terms: ((dfs, dfd, dattn), (|dfs|, |dfd|, |dattn|)).
    The derivative of the leaky ReLU at s == 0 is `slope`."""
    s = fs[src] + fd[dst]
    t = de.unsqueeze(-1) * attn.unsqueeze(0) * torch.where(s > 0, torch.ones((), dtype=F64), torch.full((), slope, dtype=F64))
    da = de.unsqueeze(-1) * _lrelu(s, slope)
    tot = lambda n, idx, x: torch.zeros((n,) + tuple(x.shape[1:]), dtype=F64).index_add_(0, idx, x)
    n_src, n_dst = fs.shape[0], fd.shape[0]
    return ((tot(n_src, src, t), tot(n_dst, dst, t), da.sum(0)),
            (tot(n_src, src, t.abs()), tot(n_dst, dst, t.abs()), da.abs().sum(0)))


def logits64(src, dst, fs, fd, attn, slope):
    """The forward alone as differentiable float64 torch (gradcheck holds `logits_backward` to it)."""
    return (attn.reshape((1,) + tuple(attn.shape[-2:])) * torch.nn.functional.leaky_relu(fs[src] + fd[dst], slope)).sum(-1)


def degree_of(idx, n):
    return torch.bincount(idx, minlength=n).to(F64)


def bounds(src, dst, fs, fd, D, abs_e, abs_grads):
    """The rounding bounds of the contract, derived from the lengths: per e[k, h] (D + 3) u sum_d |attn lrelu(s)|; per gradient entry
    the same form with the row length (dfd: the in-degree, dfs: the out-degree) or E (dattn) in place of D."""
    a_fs, a_fd, a_at = abs_grads
    E = src.numel()
    deg_out, deg_in = degree_of(src, fs.shape[0]), degree_of(dst, fd.shape[0])
    return ((D + 3) * U * abs_e, (deg_out + 3).view(-1, 1, 1) * U * a_fs, (deg_in + 3).view(-1, 1, 1) * U * a_fd, (E + 3) * U * a_at)


def integer_inputs(n_src, n_dst, E, H, D, seed, lim=8, de_lim=8, de_keep=1.0):
    """Integer-valued float32 inputs of the exact tests: fs, fd in [-lim, lim], attn in [-4, 4], de in [-de_lim, de_lim] (an entry
    kept with probability de_keep, else 0).  With a slope of 0.5 or 0.25 every product is a multiple of 0.25."""
    rng = np.random.default_rng(seed)
    f = lambda lo, hi, shape: torch.from_numpy(rng.integers(lo, hi + 1, shape).astype(np.float32))
    de = f(-de_lim, de_lim, (E, H))
    if de_keep < 1.0:
        de = de * torch.from_numpy((rng.random((E, H)) < de_keep).astype(np.float32))
    return f(-lim, lim, (n_src, H, D)), f(-lim, lim, (n_dst, H, D)), f(-4, 4, (H, D)), de


def normal_inputs(n_src, n_dst, E, H, D, seed):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(shape, generator=gen)
    return r(n_src, H, D), r(n_dst, H, D), r(H, D), r(E, H)


def exact_reference(g, fs, fd, attn, slope, de):
    """(e, dfs, dfd, dattn) of the exact tests as float64 tensors, after asserting that every sum that will be compared is exact in
    float32 whatever the order: its absolute terms add up to less than 2^22 (and are multiples of 0.25)."""
    src, dst = positions(g)
    f = lambda t: t.double()
    e, abs_e = logits_forward(src, dst, f(fs), f(fd), f(attn), slope)
    grads, abs_grads = logits_backward(src, dst, f(fs), f(fd), f(attn), slope, f(de))
    for t in (abs_e,) + abs_grads:
        assert t.numel() == 0 or float(t.max()) < EXACT_LIMIT, float(t.max())
    return (e,) + grads


# ------------------------------------------------------------------------------------------------ layer and stack, float64 torch
def _lin(x, p, name):
    y = x @ p[name + ".weight"].t()
    b = p.get(name + ".bias")
    return y if b is None else y + b


def edge_softmax64(dst, n_dst, e):
    """softmax of e [E, H] over the in-edges of every destination."""
    idx = dst.view(-1, 1).expand(-1, e.shape[1])
    m = torch.full((n_dst, e.shape[1]), -np.inf, dtype=e.dtype).scatter_reduce(0, idx, e.detach(), "amax", include_self=True)
    ex = torch.exp(e - m[dst])
    den = torch.zeros((n_dst, e.shape[1]), dtype=e.dtype).index_add(0, dst, ex)
    return ex / den[dst]


def gatv2_conv(conv, src, dst, n_dst, h_src, h_dst, p):
    """`GATv2Conv` (drop rates 0) in float64; p: the layer's parameters as float64 tensors keyed like its named_parameters (a shared
    fc_dst appears under fc_src only)."""
    H, D = conv._num_heads, conv._out_feats
    fs = _lin(h_src, p, "fc_src").view(-1, H, D)
    fd = _lin(h_dst, p, "fc_src" if conv.share_weights else "fc_dst").view(-1, H, D)
    a = edge_softmax64(dst, n_dst, logits64(src, dst, fs, fd, p["attn"], conv.negative_slope))
    rst = torch.zeros((n_dst, H, D), dtype=F64).index_add(0, dst, a.unsqueeze(-1) * fs[src])
    if conv.res_fc is not None:
        rst = rst + (h_dst @ p["res_fc.weight"].t() if "res_fc.weight" in p else h_dst).view(-1, H, D)
    return rst if conv.activation is None else conv.activation(rst)


def params64(module):
    return {k: v.detach().cpu().double().clone().requires_grad_() for k, v in module.named_parameters()}


def layer_params(p, i):
    pre = f"convs.{i}."
    return {k[len(pre):]: v for k, v in p.items() if k.startswith(pre)}


def gatv2_stack(model, layers, feat, p):
    """`GATv2` in eval mode (no dropout, BatchNorm by its running statistics) in float64; layers: per layer (src, dst, n_dst)."""
    h = feat
    n = len(model.convs)
    for i, (src, dst, n_dst) in enumerate(layers):
        h = gatv2_conv(model.convs[i], src, dst, n_dst, h, h[:n_dst], layer_params(p, i))
        if i < n - 1:
            h = h.flatten(1)
            if len(model.norms):
                bn = model.norms[i]
                h = (h - bn.running_mean.cpu().double()) * torch.rsqrt(bn.running_var.cpu().double() + bn.eps) * p[f"norms.{i}.weight"] + p[f"norms.{i}.bias"]
            h = torch.relu(h)
    return h.mean(1)


# ------------------------------------------------------------------------------------------------ shared checks
def edge_lists(g):
    src, dst = (t.cpu().long() for t in g.edges())
    return src, dst, g.number_of_src_nodes(), g.number_of_dst_nodes()


def loop_graph(n_dst, n_src, seed, chunk=None):
    """A random graph without zero in-degree: every destination gets its own row as a source plus 0 .. 6 random ones; n_src > n_dst
    makes it a block."""
    import bot_amd
    rng = np.random.default_rng(seed)
    deg = rng.integers(0, 7, n_dst)
    dst = np.concatenate([np.arange(n_dst), np.repeat(np.arange(n_dst), deg)])
    src = np.concatenate([np.arange(n_dst), rng.integers(0, n_src, int(deg.sum()))])
    order = rng.permutation(dst.size)
    return bot_amd.Graph(torch.from_numpy(src[order]), torch.from_numpy(dst[order]), n_src, num_dst_nodes=n_dst, chunk=chunk)


def check_op(g, dev, H, D, seed, slope=0.2, order="csc", impl=None, worst=None):
    """`ops.gatv2_logits` forward and the three gradients on seeded normal inputs against float64 under the derived bounds; returns the
    device results (e, dfs, dfd, dattn) and the bounds.  `worst`: a dict that collects the largest error as a fraction of its bound."""
    from bot_amd import ops
    src, dst = positions(g)
    E = src.numel()
    fs, fd, attn, de = normal_inputs(g.number_of_src_nodes(), g.number_of_dst_nodes(), E, H, D, seed)
    want_e, abs_e = logits_forward(src, dst, fs.double(), fd.double(), attn.double(), slope)
    want, abs_g = logits_backward(src, dst, fs.double(), fd.double(), attn.double(), slope, de.double())
    bnd = bounds(src, dst, fs, fd, D, abs_e, abs_g)
    leaves = [t.clone().to(dev).requires_grad_() for t in (fs, fd, attn.view(1, H, D))]
    e = ops.gatv2_logits(g, *leaves, negative_slope=slope, order=order, impl=impl)
    assert e.shape == (E, H, 1) and e.dtype == torch.float32
    eid = g.csc.eid.cpu().long()
    up = de
    if order == "eid":                       # de was drawn per position: hand it over per edge id
        up = torch.empty_like(de)
        up[eid] = de
    e.backward(up.view(E, H, 1).to(dev))
    got_e = e.detach().cpu().double().view(E, H)
    if order == "eid":
        got_e = got_e[eid]
    got = (got_e, leaves[0].grad.cpu().double(), leaves[1].grad.cpu().double(), leaves[2].grad.cpu().double().view(H, D))
    for name, a, b, lim in zip(("e", "dfs", "dfd", "dattn"), got, (want_e,) + want, bnd):
        err = (a - b).abs()
        if worst is not None and err.numel():
            frac = float((err / lim.clamp(min=1e-300)).max())
            worst[name] = max(worst.get(name, 0.0), frac)
        assert bool((err <= lim).all()), (name, H, D, float((err / lim.clamp(min=1e-300)).max()))
    return got, bnd


def make_conv(fin, H, D, seed, **kw):
    """A GATv2Conv with seeded weights and non-zero biases."""
    from bot_amd import nn as bnn
    torch.manual_seed(seed)
    conv = bnn.GATv2Conv(fin, D, H, **kw)
    gen = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for name, prm in conv.named_parameters():
            if name.endswith("bias"):
                prm.copy_(torch.randn(prm.shape, generator=gen))
    return conv


def check_conv(g, dev, fin, H, D, seed=0, pair=False, **kw):
    """One `GATv2Conv` forward + backward on `g` against `gatv2_conv` under the suite's own criteria (tests/parity_cases.py): the
    output, and the gradients of the input(s) and of every parameter.  pair: the layer takes a (feat_src, feat_dst) pair."""
    from tests.parity_cases import fwd_close, grad_close
    src, dst, n_src, n_dst = edge_lists(g)
    fin_src, fin_dst = fin if isinstance(fin, tuple) else (fin, fin)
    conv = make_conv(fin, H, D, seed, **kw).to(dev)
    gen = torch.Generator().manual_seed(seed + 1)
    x_src = torch.randn(n_src, fin_src, generator=gen)
    x_dst = torch.randn(n_dst, fin_dst, generator=gen) if pair else None
    dout = torch.randn(n_dst, H, D, generator=gen)
    xs = x_src.clone().to(dev).requires_grad_()
    xd = None if x_dst is None else x_dst.clone().to(dev).requires_grad_()
    out = conv(g, (xs, xd) if pair else xs)
    assert out.shape == (n_dst, H, D)
    out.backward(dout.to(dev))
    p = params64(conv)
    s64 = x_src.double().requires_grad_()
    d64 = None if x_dst is None else x_dst.double().requires_grad_()
    ref = gatv2_conv(conv, src, dst, n_dst, s64, s64[:n_dst] if d64 is None else d64, p)
    ref.backward(dout.double())
    fwd_close(out, ref.detach().numpy())
    grad_close(xs.grad, s64.grad.numpy())
    if pair:
        grad_close(xd.grad, d64.grad.numpy())
    for name, prm in conv.named_parameters():
        grad_close(prm.grad, p[name].grad.numpy())
    return conv


def check_stack(model, graphs, feat, dev):
    """`GATv2` in eval mode on a Graph (graphs: the graph) or a block list against `gatv2_stack`: output, input gradient and every
    parameter's gradient."""
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
    ref = gatv2_stack(model, layers, f64, p)
    ref.backward(dout.double())
    fwd_close(out, ref.detach().numpy())
    grad_close(x.grad, f64.grad.numpy())
    for name, prm in model.named_parameters():
        grad_close(prm.grad, p[name].grad.numpy())
