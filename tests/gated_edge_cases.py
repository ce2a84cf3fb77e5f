"""Float64 restatements of the contracts of the gated aggregation with an edge stream (include/bot_gnn.h "Gated aggregation
with an edge stream"), shared by tests/test_gated_edge_host.py and tests/test_gated_edge_gpu.py: the forward and the four gradients dk,
dq, dv, dc written from the formulas (no autograd) with their absolute-term sums, the rounding bounds, the `GatedGCNConv` layer and the
`GatedGCN` stack as differentiable float64 torch written from DGL's formula (separate [E, F] gathers, no merged projection), input
generators and the `check_*` functions.  The restatements call nothing of the code under test.  All per-edge tensors here are in CSC
POSITION order: (src, dst) = `positions(g)`.

The rounding bounds (U = 2^-24; gamma(c) = c U / (1 - c U)), derived in the manner of tests/gated_cases.py, never taken from a measured
error.  For the position j with s = k[w] + q[u] + c[j] and S = |k[w]| + |q[u]| + |c[j]|:
  e            the stored s_hat is the rounded sum of three terms, two additions: |s_hat - s| <= gamma(2) S.
  the gate     g and gbar leave the kernel within GATE_UNITS = 8 U of sigmoid(s_hat) and its complement (tests/gated_cases.py), and since
               |d ln g / ds| <= 1 and |d ln gbar / ds| <= 1 the error of s_hat moves either by a factor within e^(gamma(2) S): 2 S more
               units, in place of that file's |s|.  g' = g gbar: 2 GATE_UNITS + 1 + 2 S units (|d ln g' / ds| = |gbar - g| <= 1).  The
               backward forms the gate from the STORED float32 e, the same s_hat: the same count.
  a term       of ds: g' (v a + b) - the parenthesis one rounding against |v a| + |b|, the product with g' one more, the tensor form's
               chain one more: T = 2 GATE_UNITS + 2 S + 4 units on g' (|v a| + |b|).
  ds           one rounding more than that term, for the addition of de: gamma(T + 1) g' (|v a| + |b|) + U |de|.
  a sum        over a row of n positions rounds a term at most n + 1 times (chunks and the slot-order fold included).
so per output entry, with n the row's length (in-degree for num, den and dk; out-degree for dq and dv):
  num      sum_j gamma(GATE_UNITS + 2 S_j + n + 2) g_j |v_j|             den   sum_j gamma(GATE_UNITS + 2 S_j + n + 1) g_j
  dk, dq   sum_j [gamma(T_j + n + 2) g'_j (|v_j a| + |b|) + gamma(n + 2) |de_j|]
  dv       sum_j gamma(GATE_UNITS + 2 S_j + n + 2) g_j |a_j|
  out = num / (den + eps):  (b_num + |out| b_den) / (den + eps - b_den) + 2 U |out|
The tensor form's backward (torch's sigmoid_backward) forms the complement as 1 - g_hat, an ABSOLUTE error: every ds term gets
g_j (gamma(GATE_UNITS + 2 S_j) g_j + U) (|v_j a| + |b|) on top (`complement="subtracted"`)."""
import os

import numpy as np
import torch

from tests.gated_cases import EXACT_LIMIT, F64, GATE_UNITS, U, _record, _tot, gamma, gate64  # noqa: F401 - the gate's own restatement
from tests.gatv2_cases import degree_of, edge_lists, params64, positions  # noqa: F401 - shared helpers


# ------------------------------------------------------------------------------------------------ the op
def forward64(src, dst, k, q, v, c, normalize=True, eps=1e-6, drop_last_of=None, gate_error=0.0, c_late=False):
    """The forward in float64 -> dict(e, num, den, out, abs_num).  `drop_last_of` (a destination whose last in-edge is left out),
    `gate_error` (a relative error on every gate) and `c_late` (c read one position late) are the planted mistakes the bounds catch."""
    n_dst = k.shape[0]
    if c_late:
        c = torch.roll(c, 1, 0)
    e = k[dst] + q[src] + c
    g = gate64(e)[0] * (1.0 + gate_error)
    if drop_last_of is not None:
        g = g.clone()
        g[int(torch.nonzero(dst == drop_last_of).max())] = 0.0
    num, den = _tot(n_dst, dst, g * v[src]), _tot(n_dst, dst, g)
    has = degree_of(dst, n_dst).view(-1, 1) > 0
    out = torch.where(has, num / (den + eps), torch.zeros((), dtype=F64)) if normalize else num
    return dict(e=e, num=num, den=den, out=out, abs_num=_tot(n_dst, dst, g * v[src].abs()))


def backward64(src, dst, e, v, a, b=None, de=None, n_src=None, ignore_de=False):
    """The gradients from the contract's formulas: dict(ds, dk, dq, dv) - ds is dc - with a (and b, or None) float64 [n_dst, F], de
    float64 [E, F] or None.  `ignore_de`: the planted mistake."""
    n_dst, n_src = a.shape[0], v.shape[0] if n_src is None else n_src
    g, gbar = gate64(e)
    m = v[src] * a[dst] + (0 if b is None else b[dst])
    ds = g * gbar * m
    if de is not None and not ignore_de:
        ds = ds + de
    return dict(ds=ds, dk=_tot(n_dst, dst, ds), dq=_tot(n_src, src, ds), dv=_tot(n_src, src, g * a[dst]))


def upstream64(dout, out, den, normalize, eps):
    """(a, b) as the autograd op forms them from the incoming gradient."""
    if not normalize:
        return dout, None
    a = dout / (den + eps)
    return a, -a * out


def gated_edge64(src, dst, k, q, v, c, normalize=True, eps=1e-6):
    """(out, e) as differentiable float64 torch (gradcheck holds `backward64` to it)."""
    n_dst = k.shape[0]
    e = k[dst] + q[src] + c
    g = torch.sigmoid(e)
    zeros = torch.zeros((n_dst, k.shape[1]), dtype=k.dtype)
    num = zeros.index_add(0, dst, g * v[src])
    if not normalize:
        return num, e
    den = zeros.index_add(0, dst, g)
    return torch.where(degree_of(dst, n_dst).view(-1, 1) > 0, num / (den + eps), zeros), e


def bounds(src, dst, k, q, v, c, a, b=None, de=None, eps=1e-6, complement="direct"):
    """The derived rounding bounds (module docstring) -> dict(e, num, den, out, ds, dk, dq, dv); `out` is the normalised output's.  All
    operands float64."""
    n_dst, n_src = k.shape[0], q.shape[0]
    S = k[dst].abs() + q[src].abs() + c.abs()
    g, gbar = gate64(k[dst] + q[src] + c)
    gp = g * gbar
    n_in, n_out = degree_of(dst, n_dst)[dst].view(-1, 1), degree_of(src, n_src)[src].view(-1, 1)
    va, aa = v[src].abs(), a[dst].abs()
    mabs = va * aa + (0 if b is None else b[dst].abs())
    dea = torch.zeros_like(mabs) if de is None else de.abs()
    extra = g * (gamma(GATE_UNITS + 2 * S) * g + U) * mabs if complement == "subtracted" else torch.zeros_like(mabs)
    T = 2 * GATE_UNITS + 2 * S + 4
    fwd = forward64(src, dst, k, q, v, c, True, eps)
    b_num = _tot(n_dst, dst, gamma(GATE_UNITS + 2 * S + n_in + 2) * g * va)
    b_den = _tot(n_dst, dst, gamma(GATE_UNITS + 2 * S + n_in + 1) * g)
    b_out = (b_num + fwd["out"].abs() * b_den) / (fwd["den"] + eps - b_den).clamp(min=1e-300) + 2 * U * fwd["out"].abs()
    return dict(e=gamma(2) * S, num=b_num, den=b_den, out=b_out,
                ds=gamma(T + 1) * gp * mabs + U * dea + extra,
                dk=_tot(n_dst, dst, gamma(T + n_in + 2) * gp * mabs + gamma(n_in + 2) * dea + extra),
                dq=_tot(n_src, src, gamma(T + n_out + 2) * gp * mabs + gamma(n_out + 2) * dea + extra),
                dv=_tot(n_src, src, gamma(GATE_UNITS + 2 * S + n_out + 2) * g * aa))


def normal_inputs(n_src, n_dst, E, F, seed):
    """Seeded standard-normal (k, q, v, c, a, b, de): a and b stand for the incoming gradient's two dense products."""
    gen = torch.Generator().manual_seed(seed)
    r = lambda n: torch.randn((n, F), generator=gen)
    return r(n_dst), r(n_src), r(n_src), r(E), r(n_dst), r(n_dst), r(E)


REGIME_S = (0.0, 128.0, -128.0)                      # s = 0: gates 0.5, g' = 0.25;  s >= 105: gates 1, g' = 0;  s <= -105: gates 0, g' = 0
REGIME_G = {0.0: (0.5, 0.25), 128.0: (1.0, 0.0), -128.0: (0.0, 0.0)}


def exact_inputs(src, dst, n_src, n_dst, F, seed, lim=8):
    """Integer-valued float32 (k, q, v, c, a, b, de, s): k, q in [-8, 8], v, a, b, de in [-lim, lim], and c chosen per position and
    column so that s = (k + q) + c is exactly one of REGIME_S (every addition exact: small integers)."""
    rng = np.random.default_rng(seed)
    f = lambda lo, hi, n: torch.from_numpy(rng.integers(lo, hi + 1, (n, F)).astype(np.float32))
    E = src.numel()
    k, q, v = f(-8, 8, n_dst), f(-8, 8, n_src), f(-lim, lim, n_src)
    a, b, de = f(-lim, lim, n_dst), f(-lim, lim, n_dst), f(-lim, lim, E)
    s = torch.tensor(REGIME_S, dtype=torch.float32)[torch.from_numpy(rng.integers(0, 3, (E, F)))]
    c = s - (k[dst] + q[src])
    return k, q, v, c, a, b, de, s


def exact_reference(src, dst, n_src, n_dst, s, v, a, b=None, de=None):
    """What the exact regimes give, from each position's gate value alone, in float64: dict(e, num, den, ds, dk, dq, dv), after asserting
    that every sum is exact in float32 whatever its order (absolute terms below 2^22, multiples of 0.25)."""
    s, v, a = s.double(), v.double(), a.double()
    g, gp = torch.zeros_like(s), torch.zeros_like(s)
    for val, (gv, gpv) in REGIME_G.items():
        g = torch.where(s == val, torch.full_like(s, gv), g)
        gp = torch.where(s == val, torch.full_like(s, gpv), gp)
    m = v[src] * a[dst] + (0 if b is None else b.double()[dst])
    mabs = (v[src] * a[dst]).abs() + (0 if b is None else b.double()[dst].abs())
    ds = gp * m + (0 if de is None else de.double())
    dsabs = gp * mabs + (0 if de is None else de.double().abs())
    for t in (_tot(n_dst, dst, v[src].abs()), _tot(n_dst, dst, dsabs), _tot(n_src, src, dsabs), _tot(n_src, src, a[dst].abs())):
        assert t.numel() == 0 or float(t.max()) < EXACT_LIMIT, float(t.max())
    return dict(e=s, num=_tot(n_dst, dst, g * v[src]), den=_tot(n_dst, dst, g), ds=ds, dk=_tot(n_dst, dst, ds), dq=_tot(n_src, src, ds),
                dv=_tot(n_src, src, g * a[dst]))


# ------------------------------------------------------------------------------------------------ layer and stack, float64 torch
def _lin(x, p, name):
    return x @ p[name + ".weight"].t() + p[name + ".bias"]


def _bn64(x, bn, p, name):
    """BatchNorm1d in float64: batch statistics in training mode (biased variance), the running ones in eval mode."""
    if bn.training:
        mu, var = x.mean(0), x.var(0, unbiased=False)
    else:
        mu, var = bn.running_mean.cpu().double(), bn.running_var.cpu().double()
    return (x - mu) * torch.rsqrt(var + bn.eps) * p[name + ".weight"] + p[name + ".bias"]


def gatedgcn_conv64(conv, src, dst, n_dst, h_src, h_dst, e_in, p, edge_out=True):
    """`GatedGCNConv` (dropout 0) in float64 from DGL's formula; p: the layer's parameters as float64 tensors keyed like its
    named_parameters; e_in in CSC position order -> (h, e or None)."""
    Dh, Bh, Eh, Ce = _lin(h_src, p, "D"), _lin(h_src, p, "B"), _lin(h_dst, p, "E"), _lin(e_in, p, "C")
    e_hat = Dh[src] + Eh[dst] + Ce
    sig = torch.sigmoid(e_hat)
    zeros = torch.zeros((n_dst, Dh.shape[1]), dtype=F64)
    h = _lin(h_dst, p, "A") + zeros.index_add(0, dst, sig * Bh[src]) / (zeros.index_add(0, dst, sig) + 1e-6)

    def stream(x, bn, name, x_in):
        if conv.batch_norm:
            x = _bn64(x, bn, p, name)
        if conv.activation is not None:
            x = conv.activation(x)
        return x_in + x if conv.residual else x
    return stream(h, conv.bn_node, "bn_node", h_dst), (stream(e_hat, conv.bn_edge, "bn_edge", e_in) if edge_out else None)


def gatedgcn_stack64(model, src, dst, n, feat, efeat, p):
    """`GatedGCN` (dropout 0) in float64; efeat: the raw edge features in CSC position order."""
    h, e = _lin(feat, p, "embedding_h"), _lin(efeat, p, "embedding_e")
    L = len(model.convs)
    for i, conv in enumerate(model.convs):
        pre = f"convs.{i}."
        h, e = gatedgcn_conv64(conv, src, dst, n, h, h, e, {k[len(pre):]: t for k, t in p.items() if k.startswith(pre)}, edge_out=i < L - 1)
    return _lin(h, p, "out")


# ------------------------------------------------------------------------------------------------ shared checks
def check_op(g, dev, F, seed, impl=None, normalize=True, eps=1e-6, worst=None, with_de=True):
    """`ops.gated_edge_sum(order="csc")` on seeded normal inputs against float64 under the derived bounds: out (normalised: the combined
    bound), e and - unnormalised, where the incoming gradient IS a - the four gradients.  The normalised form's gradients pass through
    dense float32 ops of the autograd function (a and b), so they are held to the suite's gradient criterion (tests/parity_cases.py).
    Returns the results (out, e, dk, dq, dv, dc) as float64 CPU tensors."""
    from bot_amd import ops
    from tests.parity_cases import grad_close
    src, dst = positions(g)
    n_src, n_dst = g.number_of_src_nodes(), g.number_of_dst_nodes()
    k, q, v, c, dout, _, de = normal_inputs(n_src, n_dst, src.numel(), F, seed)
    k64, q64, v64, c64, d64 = (t.double() for t in (k, q, v, c, dout))
    de64 = de.double() if with_de else None
    fwd = forward64(src, dst, k64, q64, v64, c64, normalize, eps)
    a64, b64 = upstream64(d64, fwd["out"], fwd["den"], normalize, eps)
    want = backward64(src, dst, fwd["e"], v64, a64, b64, de64)
    tensor = (impl or os.environ.get("BOT_GATE_EDGE") or ("tensor" if str(dev) == "cpu" else ops.gate_edge_default_impl)) == "tensor"
    bnd = bounds(src, dst, k64, q64, v64, c64, a64, b64, de64, eps, complement="subtracted" if tensor else "direct")
    leaves = [t.clone().to(dev).requires_grad_() for t in (k, q, v, c)]
    out, e = ops.gated_edge_sum(g, *leaves, normalize=normalize, eps=eps, order="csc", impl=impl)
    assert out.shape == (n_dst, F) and e.shape == (src.numel(), F) and out.dtype == e.dtype == torch.float32
    torch.autograd.backward([out, e] if with_de else [out], [dout.to(dev), de.to(dev)] if with_de else [dout.to(dev)])
    got = (out.detach().cpu().double(), e.detach().cpu().double()) + tuple(t.grad.cpu().double() for t in leaves)
    tag = ("tensor " if tensor else "kernel ") + ("normalised " if normalize else "")
    pairs = (("out", fwd["out"], bnd["out" if normalize else "num"]), ("e", fwd["e"], bnd["e"]), ("dk", want["dk"], bnd["dk"]),
             ("dq", want["dq"], bnd["dq"]), ("dv", want["dv"], bnd["dv"]), ("dc", want["ds"], bnd["ds"]))
    for x, (name, y, lim) in zip(got, pairs):
        if normalize and name not in ("out", "e"):
            grad_close(x, y.numpy())
            continue
        err = (x - y).abs()
        frac = _record(worst, tag + name, err, lim)
        print(f"gated_edge_sum {tag}{name}: F={F} largest error / bound = {frac:.4f}")
        assert bool((err <= lim).all()), (tag, name, F, frac)
    return got


def make_conv(fin, fe, fout, seed, **kw):
    """A GatedGCNConv with seeded weights, non-zero biases and BatchNorm weights that do something."""
    from bot_amd import nn as bnn
    torch.manual_seed(seed)
    conv = bnn.GatedGCNConv(fin, fe, fout, **kw)
    _perturb(conv, seed)
    return conv


def _perturb(module, seed):
    gen = torch.Generator().manual_seed(seed + 100)
    with torch.no_grad():
        for name, prm in module.named_parameters():
            if name.endswith("bias"):
                prm.copy_(0.5 * torch.randn(prm.shape, generator=gen))
            elif "bn_" in name:
                prm.copy_(0.5 + torch.rand(prm.shape, generator=gen))


def check_conv(g, dev, fin, fe, fout, seed=0, order="eid", edge_out=True, **kw):
    """One `GatedGCNConv` forward + backward on `g` in training mode (batch statistics) against `gatedgcn_conv64` under the suite's own
    criteria (tests/parity_cases.py): both outputs, and the gradients of both inputs and of every parameter that takes part."""
    from tests.parity_cases import fwd_close, grad_close
    src, dst = positions(g)
    n_src, n_dst, E = g.number_of_src_nodes(), g.number_of_dst_nodes(), src.numel()
    conv = make_conv(fin, fe, fout, seed, **kw).to(dev).train()
    gen = torch.Generator().manual_seed(seed + 1)
    x, ef = torch.randn(n_src, fin, generator=gen), torch.randn(E, fe, generator=gen)           # ef: position order
    # upstream gradients at the scale of a mean loss: the biases in front of a BatchNorm have an analytically ZERO gradient, which the
    # suite's criterion holds to an absolute noise level
    dh, de = torch.randn(n_dst, fout, generator=gen) / n_dst, torch.randn(E, fout, generator=gen) / E
    eid = g.csc.eid.cpu().long() if order == "eid" and g.csc.eid is not None and _has_edge_ids(g) else None
    to_eid = (lambda t: torch.empty_like(t).index_copy_(0, eid, t)) if eid is not None else (lambda t: t)
    xs, es = x.clone().to(dev).requires_grad_(), to_eid(ef).clone().to(dev).requires_grad_()
    h, e = conv(g, xs, es, order=order, edge_out=edge_out)
    assert h.shape == (n_dst, fout) and (e is None) == (not edge_out)
    torch.autograd.backward([h, e] if edge_out else [h], [dh.to(dev), to_eid(de).to(dev)] if edge_out else [dh.to(dev)])
    p = params64(conv)
    x64, e64 = x.double().requires_grad_(), ef.double().requires_grad_()
    rh, re = gatedgcn_conv64(conv, src, dst, n_dst, x64, x64[:n_dst], e64, p, edge_out)
    torch.autograd.backward([rh, re] if edge_out else [rh], [dh.double(), de.double()] if edge_out else [dh.double()])
    fwd_close(h, rh.detach().numpy())
    if edge_out:
        fwd_close(e, to_eid(re.detach()).numpy())
    grad_close(xs.grad, x64.grad.numpy())
    grad_close(es.grad, to_eid(e64.grad).numpy())
    for name, prm in conv.named_parameters():
        if p[name].grad is None:                 # took no part: BatchNorm switched off, bn_edge without an edge output
            assert prm.grad is None and name.startswith("bn_"), name
            continue
        grad_close(prm.grad, p[name].grad.numpy())
    return conv


def _has_edge_ids(g):
    from bot_amd import ops
    return ops._csc_edge_rows(g) is not None


def check_stack(model, g, dev):
    """`GatedGCN` in training mode without dropout on a Graph or Subgraph (features from its frames) against `gatedgcn_stack64`: the
    output and every parameter's gradient."""
    from tests.parity_cases import fwd_close, grad_close
    src, dst = positions(g)
    model = model.to(dev).train()
    _perturb(model, 7)
    model.zero_grad(set_to_none=True)
    out = model(g)
    dout = torch.randn(out.shape, generator=torch.Generator().manual_seed(12)) / out.shape[0]      # (the scale of a mean loss, as check_conv)
    out.backward(dout.to(dev))
    p = params64(model)
    feat = g.to_internal(g.ndata["feat"]).cpu().double()
    ef = g.edata["feat"].cpu().double()
    if _has_edge_ids(g):
        ef = ef[g.csc.eid.cpu().long()]
    ref = gatedgcn_stack64(model, src, dst, g.number_of_nodes(), feat, ef, p)
    ref.backward(g.to_internal(dout).double())
    fwd_close(g.to_internal(out), ref.detach().numpy())
    for name, prm in model.named_parameters():
        if p[name].grad is None:
            assert prm.grad is None and "bn_edge" in name, name
            continue
        grad_close(prm.grad, p[name].grad.numpy())
