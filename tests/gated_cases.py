"""Float64 restatements of the gated-aggregation contracts (include/bot_gnn.h "Gated aggregation"), shared by
tests/test_gated_host.py and tests/test_gated_gpu.py: the forward and the three gradients written from the formulas (no autograd), the
absolute sums the rounding bounds are made of, the bounds themselves, the `ResGatedGraphConv` layer and the `ResGatedGCN` stack as
differentiable float64 torch, input generators, and the `check_*` functions that run the op, a layer or a stack against them on whatever
device the graph lives on.  The restatements call nothing of the code under test.

The rounding bounds (U = 2^-24, the unit roundoff of float32; gamma(c) = c U / (1 - c U) bounds a product of c factors (1 + d), |d| <= U).
For the edge at position j with s = k[w] + q[u]:
  the gate     g and gbar leave the kernel within GATE_U = 8 U of sigmoid(s_hat) and 1 - sigmoid(s_hat) (4 U the exponential, 2 U more
               where its error reaches 1 + e, 1 U the addition, 1 U the division), and s_hat = s (1 + d): since |d ln g / ds| = gbar <= 1
               and |d ln gbar / ds| = g <= 1, that rounding moves either by a factor within e^(|s| U): |s| more units.  g' = g gbar is one
               more rounded product and |d ln g' / ds| = |gbar - g| <= 1: 2 GATE_U + 1 + |s| units.
  a sum        over a row of n positions rounds a term at most n + 1 times (a long row: its chunk's additions and the slot-order fold, c +
               ceil(n / c) <= n + 1), and the product (or fused multiply-add) that forms the term once more.
so per output entry, with n the row's length (in-degree for num, den and dk; out-degree for dq and dv):
  num   sum_j gamma(GATE_U/U + |s_j| + n + 2) g_j |v_j|                den   sum_j gamma(GATE_U/U + |s_j| + n + 1) g_j
  dk, dq   sum_j gamma(2 GATE_U/U + |s_j| + n + 5) g'_j (|v_j a| + |b|)      (the parenthesis is one rounding against |v a| + |b|, the product
                                                                        with g' one more, and the tensor form's chain one more)
  dv    sum_j gamma(GATE_U/U + |s_j| + n + 2) g_j |a_j|
  out = num / (den + eps):  (b_num + |out| b_den) / (den + eps - b_den) + 2 U |out|   (the sum with eps and the division)
The tensor form's backward (torch's sigmoid_backward) forms the complement as 1 - g_hat: its ABSOLUTE error is that of g_hat plus one
rounding, so every ds term gets g_j (gamma(GATE_U/U + |s_j|) g_j + U) (|v_j a| + |b|) on top (`complement="subtracted"`): the relative
bound on g' is the kernel form's alone."""
import os

import numpy as np
import torch

from tests.gatv2_cases import degree_of, edge_lists, layer_params, loop_graph, params64, positions  # noqa: F401 - shared helpers

F64 = torch.float64
U = 2.0 ** -24            # the unit roundoff of float32
GATE_UNITS = 8            # the kernel's gate error in units of U, derived above; never the measured value
EXACT_LIMIT = 2.0 ** 22   # sums of multiples of 0.25 whose absolute terms add up to less than this are exact in float32


def gamma(c):
    return c * U / (1.0 - c * U)


# ------------------------------------------------------------------------------------------------ the op
def gate64(s):
    """(g, gbar) = (sigmoid(s), 1 - sigmoid(s)) in float64, each formed directly (no cancellation in either tail)."""
    e = torch.exp(-s.abs())
    pos = s >= 0
    one = torch.ones((), dtype=s.dtype)
    return torch.where(pos, one, e) / (1 + e), torch.where(pos, e, one) / (1 + e)


def _tot(n, idx, x):
    return torch.zeros((n, x.shape[1]), dtype=x.dtype).index_add_(0, idx, x)


def forward64(src, dst, k, q, v, normalize=False, eps=1e-6, drop_last_of=None, gate_error=0.0):
    """The forward in float64 -> dict(num, den, out, abs_num, s).  k [n_dst, F], q / v [n_src, F] float64.  `drop_last_of`: a destination
    whose last in-edge is left out, `gate_error`: a relative error put on every gate - the two planted mistakes the bounds must catch."""
    n_dst = k.shape[0]
    s = k[dst] + q[src]
    g = gate64(s)[0] * (1.0 + gate_error)
    if drop_last_of is not None:
        last = int(torch.nonzero(dst == drop_last_of).max())
        g = g.clone()
        g[last] = 0.0
    num, den = _tot(n_dst, dst, g * v[src]), _tot(n_dst, dst, g)
    has = degree_of(dst, n_dst).view(-1, 1) > 0
    out = torch.where(has, num / (den + eps), torch.zeros((), dtype=F64)) if normalize else num
    return dict(num=num, den=den, out=out, abs_num=_tot(n_dst, dst, g * v[src].abs()), s=s)


def backward64(src, dst, k, q, v, a, b=None):
    """The three gradients of the contract from its formulas, and for each the sum of the absolute terms:
    ((dk, dq, dv), (|dk|, |dq|, |dv|)).  a (and b, or None) float64 [n_dst, F]."""
    n_dst, n_src = k.shape[0], q.shape[0]
    g, gbar = gate64(k[dst] + q[src])
    gp = g * gbar
    m = v[src] * a[dst] + (0 if b is None else b[dst])
    mabs = (v[src] * a[dst]).abs() + (0 if b is None else b[dst].abs())
    ds, dsabs = gp * m, gp * mabs
    return ((_tot(n_dst, dst, ds), _tot(n_src, src, ds), _tot(n_src, src, g * a[dst])),
            (_tot(n_dst, dst, dsabs), _tot(n_src, src, dsabs), _tot(n_src, src, g * a[dst].abs())))


def upstream64(dout, out, den, normalize, eps):
    """(a, b) as the autograd op forms them from the incoming gradient."""
    if not normalize:
        return dout, None
    a = dout / (den + eps)
    return a, -a * out


def gated64(src, dst, k, q, v, normalize=False, eps=1e-6):
    """The forward alone as differentiable float64 torch (gradcheck holds `backward64` to it)."""
    n_dst = k.shape[0]
    g = torch.sigmoid(k[dst] + q[src])
    zeros = torch.zeros((n_dst, k.shape[1]), dtype=k.dtype)
    num = zeros.index_add(0, dst, g * v[src])
    if not normalize:
        return num
    den = zeros.index_add(0, dst, g)
    return torch.where(degree_of(dst, n_dst).view(-1, 1) > 0, num / (den + eps), zeros)


def bounds(src, dst, k, q, v, a, b=None, eps=1e-6, complement="direct"):
    """The derived rounding bounds (module docstring) -> dict(num, den, out, dk, dq, dv); `out` is the normalised output's.  All
    operands float64."""
    n_dst, n_src = k.shape[0], q.shape[0]
    s = k[dst] + q[src]
    g, gbar = gate64(s)
    gp = g * gbar
    sa = s.abs()
    n_in, n_out = degree_of(dst, n_dst)[dst].view(-1, 1), degree_of(src, n_src)[src].view(-1, 1)
    va = v[src].abs()
    aa = a[dst].abs()
    mabs = va * aa + (0 if b is None else b[dst].abs())
    extra = g * (gamma(GATE_UNITS + sa) * g + U) * mabs if complement == "subtracted" else torch.zeros_like(mabs)
    fwd = forward64(src, dst, k, q, v, True, eps)
    b_num = _tot(n_dst, dst, gamma(GATE_UNITS + sa + n_in + 2) * g * va)
    b_den = _tot(n_dst, dst, gamma(GATE_UNITS + sa + n_in + 1) * g)
    b_out = (b_num + fwd["out"].abs() * b_den) / (fwd["den"] + eps - b_den).clamp(min=1e-300) + 2 * U * fwd["out"].abs()
    return dict(num=b_num, den=b_den, out=b_out,
                dk=_tot(n_dst, dst, gamma(2 * GATE_UNITS + sa + n_in + 5) * gp * mabs + extra),
                dq=_tot(n_src, src, gamma(2 * GATE_UNITS + sa + n_out + 5) * gp * mabs + extra),
                dv=_tot(n_src, src, gamma(GATE_UNITS + sa + n_out + 2) * g * aa))


def normal_inputs(n_src, n_dst, F, seed):
    """Seeded standard-normal (k, q, v, a, b): a and b stand for the incoming gradient's two dense products."""
    gen = torch.Generator().manual_seed(seed)
    r = lambda n: torch.randn((n, F), generator=gen)
    return r(n_dst), r(n_src), r(n_src), r(n_dst), r(n_dst)


def integer_inputs(n_src, n_dst, F, seed, lim=8):
    """Integer-valued float32 (q, v, a): q in [-8, 8], v and a in [-lim, lim]."""
    rng = np.random.default_rng(seed)
    f = lambda lo, hi, n: torch.from_numpy(rng.integers(lo, hi + 1, (n, F)).astype(np.float32))
    return f(-8, 8, n_src), f(-lim, lim, n_src), f(-lim, lim, n_dst)


def exact_reference(g, regime, v, a):
    """What the three exact regimes of the contract give, from the regime's gate value alone (float64 tensors): (out, dk, dq, dv) of the
    unnormalised form for gates 1 (g' = 0), 0 (g' = 0) and 0.5 (g' = 0.25), after asserting that every sum is exact in float32 whatever
    its order (absolute terms below 2^22, multiples of 0.25)."""
    src, dst = positions(g)
    n_src, n_dst = g.number_of_src_nodes(), g.number_of_dst_nodes()
    gate, gp = {"one": (1.0, 0.0), "zero": (0.0, 0.0), "half": (0.5, 0.25)}[regime]
    v, a = v.double(), a.double()
    va = v[src] * a[dst]
    for t in (_tot(n_dst, dst, v[src].abs()), _tot(n_dst, dst, va.abs()), _tot(n_src, src, va.abs()), _tot(n_src, src, a[dst].abs())):
        assert t.numel() == 0 or float(t.max()) < EXACT_LIMIT, float(t.max())
    return (gate * _tot(n_dst, dst, v[src]), gp * _tot(n_dst, dst, va), gp * _tot(n_src, src, va), gate * _tot(n_src, src, a[dst]))


# ------------------------------------------------------------------------------------------------ layer and stack, float64 torch
def _lin(x, p, name):
    y = x @ p[name + ".weight"].t()
    b = p.get(name + ".bias")
    return y if b is None else y + b


def gated_conv64(conv, src, dst, n_dst, h_src, h_dst, p):
    """`ResGatedGraphConv` (feat_drop 0) in float64; p: the layer's parameters as float64 tensors keyed like its named_parameters."""
    out = gated64(src, dst, _lin(h_dst, p, "lin_key"), _lin(h_src, p, "lin_query"), _lin(h_src, p, "lin_value"), conv.normalize, conv.eps)
    if "lin_skip.weight" in p:
        out = out + h_dst @ p["lin_skip.weight"].t()
    if "bias" in p:
        out = out + p["bias"]
    return out if conv.activation is None else conv.activation(out)


def gated_stack64(model, layers, feat, p):
    """`ResGatedGCN` in eval mode (no dropout, BatchNorm by its running statistics) in float64; layers: per layer (src, dst, n_dst)."""
    h = feat
    n = len(model.convs)
    for i, (src, dst, n_dst) in enumerate(layers):
        h = gated_conv64(model.convs[i], src, dst, n_dst, h, h[:n_dst], layer_params(p, i))
        if i < n - 1:
            if len(model.norms):
                bn = model.norms[i]
                h = (h - bn.running_mean.cpu().double()) * torch.rsqrt(bn.running_var.cpu().double() + bn.eps) * p[f"norms.{i}.weight"] + p[f"norms.{i}.bias"]
            h = torch.relu(h)
    return h


# ------------------------------------------------------------------------------------------------ shared checks
def _record(worst, name, err, lim):
    frac = float((err / lim.clamp(min=1e-300)).max()) if err.numel() else 0.0
    if worst is not None:
        worst[name] = max(worst.get(name, 0.0), frac)
    return frac


def check_op(g, dev, F, seed, impl=None, normalize=False, eps=1e-6, worst=None):
    """`ops.gated_sum` on seeded normal inputs against float64 under the derived bounds: the output (normalised: under the combined
    bound) and - unnormalised, where the incoming gradient IS a - the three gradients.  The normalised form's gradients pass through
    dense float32 ops of the autograd function (a and b), so they are held to the suite's gradient criterion (tests/parity_cases.py).
    Returns the device results (out, dk, dq, dv) as float64 CPU tensors and the bounds."""
    from bot_amd import ops
    from tests.parity_cases import grad_close
    src, dst = positions(g)
    k, q, v, dout, _ = normal_inputs(g.number_of_src_nodes(), g.number_of_dst_nodes(), F, seed)
    k64, q64, v64, d64 = (t.double() for t in (k, q, v, dout))
    fwd = forward64(src, dst, k64, q64, v64, normalize, eps)
    a64, b64 = upstream64(d64, fwd["out"], fwd["den"], normalize, eps)
    want, _ = backward64(src, dst, k64, q64, v64, a64, b64)
    # the form that runs, as the op documents its choice: the argument, else the BOT_GATE variable, else the default for the device
    tensor = (impl or os.environ.get("BOT_GATE") or ("tensor" if str(dev) == "cpu" else ops.gate_default_impl)) == "tensor"
    bnd = bounds(src, dst, k64, q64, v64, a64, b64, eps, complement="subtracted" if tensor else "direct")
    leaves = [t.clone().to(dev).requires_grad_() for t in (k, q, v)]
    out = ops.gated_sum(g, *leaves, normalize=normalize, eps=eps, impl=impl)
    assert out.shape == (g.number_of_dst_nodes(), F) and out.dtype == torch.float32
    out.backward(dout.to(dev))
    got = (out.detach().cpu().double(),) + tuple(t.grad.cpu().double() for t in leaves)
    lims = (bnd["out" if normalize else "num"], bnd["dk"], bnd["dq"], bnd["dv"])
    tag = ("tensor " if tensor else "kernel ") + ("normalised " if normalize else "")
    for name, x, y, lim in zip(("out", "dk", "dq", "dv"), got, (fwd["out"],) + want, lims):
        if normalize and name != "out":
            grad_close(x, y.numpy())
            continue
        err = (x - y).abs()
        frac = _record(worst, tag + name, err, lim)
        print(f"gated_sum {tag}{name}: F={F} largest error / bound = {frac:.4f}")
        assert bool((err <= lim).all()), (tag, name, F, frac)
    return got, lims


def make_conv(fin, fout, seed, **kw):
    """A ResGatedGraphConv with seeded weights and non-zero biases."""
    from bot_amd import nn as bnn
    torch.manual_seed(seed)
    conv = bnn.ResGatedGraphConv(fin, fout, **kw)
    gen = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for name, prm in conv.named_parameters():
            if name.endswith("bias"):
                prm.copy_(torch.randn(prm.shape, generator=gen))
    return conv


def check_conv(g, dev, fin, fout, seed=0, pair=False, **kw):
    """One `ResGatedGraphConv` forward + backward on `g` against `gated_conv64` under the suite's own criteria (tests/parity_cases.py):
    the output, and the gradients of the input(s) and of every parameter.  pair: the layer takes a (feat_src, feat_dst) pair."""
    from tests.parity_cases import fwd_close, grad_close
    src, dst, n_src, n_dst = edge_lists(g)
    fin_src, fin_dst = fin if isinstance(fin, tuple) else (fin, fin)
    conv = make_conv(fin, fout, seed, **kw).to(dev)
    gen = torch.Generator().manual_seed(seed + 1)
    x_src = torch.randn(n_src, fin_src, generator=gen)
    x_dst = torch.randn(n_dst, fin_dst, generator=gen) if pair else None
    dout = torch.randn(n_dst, fout, generator=gen)
    xs = x_src.clone().to(dev).requires_grad_()
    xd = None if x_dst is None else x_dst.clone().to(dev).requires_grad_()
    out = conv(g, (xs, xd) if pair else xs)
    assert out.shape == (n_dst, fout)
    out.backward(dout.to(dev))
    p = params64(conv)
    s64 = x_src.double().requires_grad_()
    d64 = None if x_dst is None else x_dst.double().requires_grad_()
    ref = gated_conv64(conv, src, dst, n_dst, s64, s64[:n_dst] if d64 is None else d64, p)
    ref.backward(dout.double())
    fwd_close(out, ref.detach().numpy())
    grad_close(xs.grad, s64.grad.numpy())
    if pair:
        grad_close(xd.grad, d64.grad.numpy())
    for name, prm in conv.named_parameters():
        grad_close(prm.grad, p[name].grad.numpy())
    return conv


def check_stack(model, graphs, feat, dev):
    """`ResGatedGCN` in eval mode on a Graph (graphs: the graph) or a block list against `gated_stack64`: output, input gradient and
    every parameter's gradient."""
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
    ref = gated_stack64(model, layers, f64, p)
    ref.backward(dout.double())
    fwd_close(out, ref.detach().numpy())
    grad_close(x.grad, f64.grad.numpy())
    for name, prm in model.named_parameters():
        grad_close(prm.grad, p[name].grad.numpy())
