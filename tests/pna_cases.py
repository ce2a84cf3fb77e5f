"""Float64 restatements of the PNA contracts (include/bot_gnn.h "PNA aggregation"), shared by tests/test_pna_host.py and
tests/test_pna_gpu.py: the aggregators over the full message a[u] + b[v], the scalers, the tower layout, the owner positions of max and
min, the autograd of the same formula with its var == 0 gate, and `PNAConv` / `PNA`.  The restatements call nothing of the code under
test; the `check_*` functions at the end run an op, a layer or a stack against them on whatever device the graph lives on.  The graphs,
the tie values and the position checks are tests/sage_cases.py's."""
import math

import numpy as np
import torch

from tests import sage_cases as SG

F64 = torch.float64
U32 = 2.0 ** -24                      # float32's unit roundoff
AGGS4 = ("mean", "max", "min", "std")
SCALERS3 = ("identity", "amplification", "attenuation")


# ------------------------------------------------------------------------------------------------ the aggregation, numpy float64
def scale_table(indptr, scalers, delta):
    """float64 [S, n]: identity 1, amplification log(n + 1) / delta, attenuation delta / log(n + 1); 0 for an empty row."""
    deg = np.diff(np.asarray(indptr, dtype=np.int64))
    L = np.log(deg + 1.0)
    rows = {"identity": np.ones_like(L), "amplification": L / delta, "attenuation": delta / np.where(deg > 0, L, 1.0)}
    return np.stack([np.where(deg > 0, rows[s], 0.0) for s in scalers])


def layout(vals, scale, Ft):
    """[A, n, F] aggregator values and [S, n] scalers -> [n, S*A*F]: column tower * S*A*Ft + (s*A + a) * Ft + f, written as loops."""
    A, n, F = vals.shape
    S, T = scale.shape[0], F // Ft
    out = np.zeros((n, S * A * F), dtype=np.float64)
    for t in range(T):
        for s in range(S):
            for a in range(A):
                c0 = t * S * A * Ft + (s * A + a) * Ft
                out[:, c0:c0 + Ft] = scale[s][:, None] * vals[a][:, t * Ft:(t + 1) * Ft]
    return out


def owners(indptr, indices, a):
    """(argmax, argmin) int32 [n, F]: the smallest CSC position that attains the max / the min of a over the row (numeric ties:
    -0.0 == +0.0), -1 on an empty row.  a keeps its dtype: a compare does not round."""
    _, amax = SG.max_forward(indptr, indices, a)
    _, amin = SG.max_forward(indptr, indices, -a)
    return amax, amin


def aggregate(indptr, indices, a, b, aggregators):
    """The aggregators of m_k = a[u_k] + b[v] per row in float64, computed on the messages themselves (two passes for the variance), and
    what the error bounds of the issue need.  Returns (vals {name: [n, F]}, info) with info: deg [n], p [n, F] (the first neighbour's row of
    a), dmax [n, F] = max_k |a_k - p|, asum [n, F] = sum_k |a_k|, and `bvals` the |b| rows.  Empty rows are 0."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    n, F = len(indptr) - 1, a.shape[1]
    a64 = a.astype(np.float64)
    b64 = np.zeros((n, F)) if b is None else b.astype(np.float64)
    names = ("mean", "sum", "max", "min", "std", "var")
    vals = {k: np.zeros((n, F)) for k in names}
    info = {k: np.zeros((n, F)) for k in ("p", "dmax", "asum")}
    info["deg"], info["babs"] = np.diff(indptr), np.abs(b64)
    for r in range(n):
        lo, hi = indptr[r], indptr[r + 1]
        if hi == lo:
            continue
        rows = a64[indices[lo:hi]]
        m = rows + b64[r]
        mean = m.mean(0)
        var = np.maximum(((m - mean) ** 2).mean(0), 0.0)
        vals["mean"][r], vals["sum"][r], vals["max"][r], vals["min"][r] = mean, m.sum(0), m.max(0), m.min(0)
        vals["var"][r], vals["std"][r] = var, np.sqrt(var + 1e-30)
        info["p"][r], info["dmax"][r], info["asum"][r] = rows[0], np.abs(rows - rows[0]).max(0), np.abs(rows).sum(0)
    return {k: vals[k] for k in aggregators}, vals, info


def pna_forward(indptr, indices, a, b, aggregators, scalers, delta, Ft=None):
    """out float64 [n, S*A*F] of the contract, with (argmax, argmin)."""
    chosen, _, _ = aggregate(indptr, indices, a, b, aggregators)
    vals = np.stack([chosen[k] for k in aggregators])
    return layout(vals, scale_table(indptr, scalers, delta), Ft or a.shape[1]), owners(indptr, indices, a)


# ------------------------------------------------------------------------------------------------ the same formula, float64 autograd
def pna_torch(indptr, indices, a, b, aggregators, scalers, delta, Ft=None, argmax=None, argmin=None):
    """The contract as differentiable float64 torch ops.  var is the mean of the squared deviations (equal to mean m^2 - mean(m)^2,
    and exactly 0 on a constant row), through relu - whose gradient at 0 is 0: the var == 0 gate.  With `argmax` / `argmin` ([n, F] CSC
    positions, -1 = none) max and min are evaluated AT those owners - the function whose gradient is the kernel's routing."""
    indptr_t = torch.as_tensor(np.asarray(indptr, dtype=np.int64))
    idx = torch.as_tensor(np.asarray(indices, dtype=np.int64))
    n, F = indptr_t.numel() - 1, a.shape[1]
    deg = indptr_t[1:] - indptr_t[:-1]
    seg = torch.repeat_interleave(torch.arange(n), deg)
    some = (deg > 0).reshape(-1, 1)
    cnt = deg.clamp(min=1).to(F64).reshape(-1, 1)
    zero = torch.zeros((), dtype=F64)
    bb = torch.zeros((n, F), dtype=F64) if b is None else b
    msg = a[idx] + bb[seg]
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
    scale = torch.from_numpy(scale_table(indptr, scalers, delta))                              # [S, n]
    S, A, Ft = scale.shape[0], len(aggregators), Ft or F
    v = vals.reshape(n, 1, A, F // Ft, Ft) * scale.t().reshape(n, S, 1, 1, 1)
    return v.permute(0, 3, 1, 2, 4).reshape(n, S * A * F)


# ------------------------------------------------------------------------------------------------ PNAConv and PNA, float64
def _lin(x, p, name):
    return x @ p[name + ".weight"].t() + p[name + ".bias"]


def _bn(z, p, pre, bn, training):
    if training:
        mean, var = z.mean(0), z.var(0, unbiased=False)
    else:
        mean, var = bn.running_mean.detach().cpu().double(), bn.running_var.detach().cpu().double()
    return (z - mean) * torch.rsqrt(var + bn.eps) * p[pre + ".weight"] + p[pre + ".bias"]


def pna_conv(conv, indptr, indices, h_src, h_dst, p, sarg=None, training=True):
    """`PNAConv` in float64 the way DGL writes it: per tower the message M(cat[h_u, h_v]) per edge, the aggregation, U(cat[h, h_neigh])
    / sqrt(n_dst), BatchNorm (batch statistics when training, no dropout); the towers side by side, the mixing layer, the residual.
    p: the layer's parameters as float64 tensors; sarg: the kernel's [n_dst, 2 F] owner positions, or None."""
    T, Ft = conv.num_towers, conv.tower_in_size
    n_dst, F = h_dst.shape[0], conv.in_size
    outs = []
    for t in range(T):
        hs, hd = h_src[:, t * Ft:(t + 1) * Ft], h_dst[:, t * Ft:(t + 1) * Ft]
        M = p[f"towers.{t}.M.weight"]
        a, b = hs @ M[:, :Ft].t(), hd @ M[:, Ft:].t() + p[f"towers.{t}.M.bias"]           # M(cat[h_u, h_v]) = a[u] + b[v]
        amax = None if sarg is None else sarg[:, t * Ft:(t + 1) * Ft]
        amin = None if sarg is None else sarg[:, F + t * Ft:F + (t + 1) * Ft]
        h_neigh = pna_torch(indptr, indices, a, b, conv.aggregators, conv.scalers, conv.delta, None, amax, amin)
        z = _lin(torch.cat([hd, h_neigh], dim=1), p, f"towers.{t}.U") / math.sqrt(n_dst)
        outs.append(_bn(z, p, f"towers.{t}.batchnorm", conv.towers[t].batchnorm, training))
    h = torch.nn.functional.leaky_relu(_lin(torch.cat(outs, dim=1), p, "mixing_layer.0"), 0.01)
    return h + h_dst if conv.residual else h


def pna_stack(model, layers, feat, p, sargs=None, training=False):
    """`PNA` (no dropout) in float64.  layers: per layer (indptr, indices, n_dst); sargs: per layer the kernel's owner positions."""
    h = _lin(feat, p, "encoder")
    for i, (indptr, indices, n_dst) in enumerate(layers):
        pre = f"convs.{i}."
        pi = {k[len(pre):]: v for k, v in p.items() if k.startswith(pre)}
        h = pna_conv(model.convs[i], indptr, indices, h, h[:n_dst], pi, None if sargs is None else sargs[i], training)
        if i < len(layers) - 1:
            h = torch.relu(h)
    return _lin(h, p, "decoder")


# ------------------------------------------------------------------------------------------------ checks shared by both suites
class Spy:
    """Records the owner positions of every `ops.pna_aggregate` call of the layers while active (the calls run with return_saved)."""

    def __init__(self, monkeypatch):
        from bot_amd import ops
        self.sarg, self.calls = [], 0
        real = getattr(ops.pna_aggregate, "real", ops.pna_aggregate)       # a second Spy of one test replaces the first

        def pna_aggregate(g, a, b=None, *args, **kw):
            kw["return_saved"] = True
            out, saved, sarg = real(g, a, b, *args, **kw)
            self.calls += 1
            self.sarg.append(sarg.cpu().numpy())
            return out
        pna_aggregate.real = real
        monkeypatch.setattr(ops, "pna_aggregate", pna_aggregate)


def randomise(module, seed):
    """Biases and BatchNorm parameters / running statistics that do something."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, prm in module.named_parameters():
            if name.endswith("bias"):
                prm.copy_(0.5 * torch.randn(prm.shape, generator=gen))
            elif "batchnorm" in name:
                prm.copy_(0.5 + torch.rand(prm.shape, generator=gen))
        for m in module.modules():
            if isinstance(m, torch.nn.BatchNorm1d):
                m.running_mean.copy_(0.3 * torch.randn(m.running_mean.shape, generator=gen))
                m.running_var.copy_(0.5 + torch.rand(m.running_var.shape, generator=gen))


def check_conv(g, dev, monkeypatch, in_size, out_size, towers, residual, aggregators=AGGS4, scalers=SCALERS3, seed=0, impl=None):
    """One `PNAConv` forward + backward in eval mode (BatchNorm by its running statistics - with batch statistics the gradient of
    U.bias is 0 in exact arithmetic and rounding noise in float32, which no relative criterion can hold) on `g` against `pna_conv`
    evaluated at the layer's own owner positions, under the suite's criteria (tests/parity_cases.py); ONE aggregation call per forward."""
    from bot_amd import nn as bnn
    from tests.parity_cases import fwd_close, grad_close
    indptr, indices = SG.csc_of(g)
    n_src, n_dst = g.number_of_src_nodes(), g.number_of_dst_nodes()
    torch.manual_seed(seed)
    conv = bnn.PNAConv(in_size, out_size, aggregators, scalers, delta=1.7, num_towers=towers, residual=residual)
    randomise(conv, seed + 1)
    conv = conv.to(dev).eval()
    gen = torch.Generator().manual_seed(seed + 2)
    feat = torch.randn(n_src, in_size, generator=gen).to(dev).requires_grad_()
    dout = torch.randn(n_dst, out_size, generator=gen)
    spy = Spy(monkeypatch)
    out = conv(g, feat) if impl is None else conv(g, feat, impl=impl)
    assert spy.calls == 1 and out.shape == (n_dst, out_size)
    out.backward(dout.to(dev))
    p = SG.params64(conv)
    f64 = feat.detach().cpu().double().requires_grad_()
    sarg = spy.sarg[0]
    SG.check_arg(indptr, sarg)
    ref = pna_conv(conv, indptr, indices, f64, f64[:n_dst], p, sarg, training=False)
    ref.backward(dout.double())
    fwd_close(out, ref.detach().numpy())
    grad_close(feat.grad, f64.grad.numpy())
    for name, prm in conv.named_parameters():
        grad_close(prm.grad, p[name].grad.numpy())
    return conv


def check_stack(model, graphs, feat, dev, monkeypatch):
    """`PNA` in eval mode on a Graph or a block list against `pna_stack` at the layers' own owner positions: output, input gradient and
    every parameter's gradient."""
    from tests.parity_cases import fwd_close, grad_close
    blocks = graphs if isinstance(graphs, (list, tuple)) else None
    per_layer = list(blocks) if blocks is not None else [graphs] * model.n_layers
    randomise(model, 5)
    model = model.to(dev).eval()
    model.zero_grad(set_to_none=True)
    x = feat.detach().clone().to(dev).requires_grad_()
    spy = Spy(monkeypatch)
    out = model(graphs, x)
    assert spy.calls == model.n_layers
    dout = torch.randn(out.shape, generator=torch.Generator().manual_seed(12))
    out.backward(dout.to(dev))
    p = SG.params64(model)
    f64 = feat.detach().cpu().double().requires_grad_()
    layers = [SG.csc_of(g) + (g.number_of_dst_nodes(),) for g in per_layer]
    ref = pna_stack(model, layers, f64, p, spy.sarg)
    ref.backward(dout.double())
    fwd_close(out, ref.detach().numpy())
    grad_close(x.grad, f64.grad.numpy())
    for name, prm in model.named_parameters():
        grad_close(prm.grad, p[name].grad.numpy())
