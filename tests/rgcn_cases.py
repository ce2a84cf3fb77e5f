"""Float64 restatements of the relation sweeps' contracts (include/bot_gnn.h "Relational aggregation"), shared by
tests/test_rgcn_host.py and tests/test_rgcn_gpu.py: expand, contract and their gradients written from the formulas (no autograd), the
absolute sums the rounding bounds are made of, the bounds themselves, `RelGraphConv` and the `RGCN` stack as differentiable float64
torch, input builders, and the `check_*` functions that run the ops, a layer or a stack against them on whatever device the graph lives
on.  The restatements call nothing of the code under test.

The edge e = (u -> v) has the relation r_e and the constant weight c_e; coef is [R, B] (one-hot mode: the identity, B = R):
  expand    Z[v, b, :]  = sum_e c_e coef[r_e, b] x[u, :]                   dx[u, :]    = sum_e c_e sum_b coef[r_e, b] dZ[v, b, :]
  contract  out[v, :]   = sum_e c_e sum_b coef[r_e, b] y[u, b, :]          dy[u, b, :] = sum_e c_e coef[r_e, b] dout[v, :]
  dcoef[r, b] = sum_{e: r_e = r} c_e <x[u], dZ[v, b, :]>   (expand),   sum_{e: r_e = r} c_e <y[u, b, :], dout[v, :]>   (contract)
so each sweep's source-side gradient is the other sweep over the transposed direction.

The rounding bounds (U = 2^-24, the unit roundoff of float32; gamma(c) = c U / (1 - c U) bounds a product of c factors (1 + d), |d| <= U).
Per output entry of a row of n positions that the row plan cuts into m chunks (m = 0 for a whole row), from the kernel's operations:
  expand     the weight c_e * coef is one rounding, every position one fused multiply-add (n), the slot-order fold of the chunks m more:
             n + m + 1 roundings at most on any term, held to gamma(n + m + 2) sum |terms|.
  contract   the sum over the blocks of a pass is a product and fused multiply-adds, min(B, 16) roundings; the fused multiply-add with
             c_e one per position AND per pass (P = ceil(B / 16) passes run on one accumulator, pass-major), the fold m more: held to
             gamma(n P + m + min(B, 16) + 2) sum |terms|, which for B <= 16 is gamma(n + m + B + 2).  One-hot: one block, one pass.
  dcoef      the dot over F columns rounds a term at most F times, the product with c_e once, the segment sum over the relation's n_r
             positions at most n_r + ceil(n_r / 64) times (its chunks are at least 64 long): gamma(F + n_r + ceil(n_r / 64) + 3).
The tensor form's counts (a weight, a product, a sum over B, an `index_add` of n terms) are no larger, so it is held to the same bounds.
A gradient is a sweep over the other direction: its n and m are that direction's.

The exact regime: x, y and the incoming gradients integer-valued, the norm in {0.25, 0.5, 1, 2}, coef multiples of 0.25 in [-2, 2].  Every
term of a sweep is then a multiple of 2^-4 and every term of dcoef a multiple of 2^-2, so float32 sums are exact, whatever their order,
while the sum of the absolute terms stays below 2^24 times that quantum; the builders assert it (and the 2^22 the contract names)."""
import numpy as np
import torch

from tests.gatv2_cases import edge_lists, layer_params, params64, positions  # noqa: F401 - shared helpers

F64 = torch.float64
U = 2.0 ** -24            # the unit roundoff of float32
PASS_BLOCKS = 16          # the sweeps' blocks per pass (csrc/spmm_rel.hip kRelBlocks)
SEG_CHUNK = 64            # the smallest chunk of a row plan (`_C.default_chunk`)


def gamma(c):
    return c * U / (1.0 - c * U)


def _tot(n, idx, x):
    return torch.zeros((n,) + tuple(x.shape[1:]), dtype=x.dtype).index_add_(0, idx, x)


def full_coef(coef, R):
    """The coefficient table the formulas use: `coef` in float64, or the identity of the one-hot mode."""
    return torch.eye(R, dtype=F64) if coef is None else coef.to(F64)


# ------------------------------------------------------------------------------------------------ the sweeps
def expand64(src, dst, et, c, coef, x, n_dst, absolute=False):
    """Z [n_dst, B, F] in float64 (absolute: the sum of the absolute terms).  src, dst, et int64 [E]; c float64 [E]; coef float64 [R, B]."""
    w = coef[et] * c.unsqueeze(1)                                              # [E, B]
    xs = x[src]
    if absolute:
        w, xs = w.abs(), xs.abs()
    return _tot(n_dst, dst, w.unsqueeze(2) * xs.unsqueeze(1))


def contract64(src, dst, et, c, coef, y, n_dst, absolute=False):
    """out [n_dst, F] in float64 (absolute: the sum of the absolute terms); y float64 [n_src, B, F]."""
    w = coef[et] * c.unsqueeze(1)
    ys = y[src]
    if absolute:
        w, ys = w.abs(), ys.abs()
    return _tot(n_dst, dst, (w.unsqueeze(2) * ys).sum(1))


def expand_grads64(src, dst, et, c, coef, x, dZ, absolute=False):
    """(dx [n_src, F], dcoef [R, B]) of expand from the formulas."""
    dx = contract64(dst, src, et, c, coef, dZ, x.shape[0], absolute)           # the transpose: contract over the reversed edges
    xs, zs = x[src], dZ[dst]
    dots = ((xs.abs().unsqueeze(1) * zs.abs()) if absolute else (xs.unsqueeze(1) * zs)).sum(2)       # [E, B]
    return dx, _tot(coef.shape[0], et, dots * (c.abs() if absolute else c).unsqueeze(1))


def contract_grads64(src, dst, et, c, coef, y, dout, absolute=False):
    """(dy [n_src, B, F], dcoef [R, B]) of contract from the formulas."""
    dy = expand64(dst, src, et, c, coef, dout, y.shape[0], absolute)
    ys, ds = y[src], dout[dst]
    dots = ((ys.abs() * ds.abs().unsqueeze(1)) if absolute else (ys * ds.unsqueeze(1))).sum(2)
    return dy, _tot(coef.shape[0], et, dots * (c.abs() if absolute else c).unsqueeze(1))


def row_counts(idx, n, chunk):
    """(n_v, m_v) per row of a direction whose row of every edge is `idx`: the length, and the chunks of a long row (0 for a whole one)."""
    deg = torch.bincount(idx, minlength=n).to(F64)
    return deg, torch.where(deg > chunk, torch.ceil(deg / chunk), torch.zeros_like(deg))


def expand_factor(idx, n, chunk):
    deg, m = row_counts(idx, n, chunk)
    return gamma(deg + m + 2)


def contract_factor(idx, n, chunk, B):
    """B: the coefficient columns (one-hot: 1, one block is gathered)."""
    deg, m = row_counts(idx, n, chunk)
    passes = -(-B // PASS_BLOCKS)
    return gamma(deg * passes + m + min(B, PASS_BLOCKS) + 2)


def dcoef_factor(et, R, Fw):
    n_r = torch.bincount(et, minlength=R).to(F64)
    return gamma(Fw + n_r + torch.ceil(n_r / SEG_CHUNK) + 3)


# ------------------------------------------------------------------------------------------------ inputs
def relations(g, R, seed):
    """int64 [E] in edge-id order: seeded uniform relations, except that the last relation has no edge (R > 1) and every in-edge of the
    longest row has relation 0."""
    _, dst, _, n_dst = edge_lists(g)
    rng = np.random.default_rng(seed)
    et = torch.from_numpy(rng.integers(0, max(R - 1, 1), dst.numel()))
    if dst.numel():
        et[dst == int(torch.argmax(torch.bincount(dst, minlength=n_dst)))] = 0
    return et


def position_order(g, t):
    """A per-edge tensor (edge-id order, CPU) in the graph's CSC position order."""
    return t[g.csc.eid.cpu().long()]


def normal_case(g, Fw, R, B, seed):
    """Seeded normal inputs: dict(x, y, dZ, dout, coef (None for B = None: one-hot), norm, et), CPU float32 / int64, edge-id order."""
    gen = torch.Generator().manual_seed(seed)
    n_src, n_dst, E = g.number_of_src_nodes(), g.number_of_dst_nodes(), g.number_of_edges()
    Bc = R if B is None else B
    r = lambda *s: torch.randn(s, generator=gen)
    return dict(x=r(n_src, Fw), y=r(n_src, Bc, Fw), dZ=r(n_dst, Bc, Fw), dout=r(n_dst, Fw), coef=None if B is None else r(R, B),
                norm=torch.rand(E, generator=gen) + 0.25, et=relations(g, R, seed + 1))


def exact_case(g, Fw, R, B, seed, lim=8):
    """The exact regime (module docstring): the same dict, x and y integers in [-lim, lim], the incoming gradients in [-lim, lim] (in [-2, 2]
    from 256 columns on, which keeps dcoef's sums small), coef multiples of 0.25 in [-2, 2], norm in {0.25, 0.5, 1, 2}; asserts that every
    sum of absolute terms is below its exactness limit."""
    rng = np.random.default_rng(seed)
    n_src, n_dst, E = g.number_of_src_nodes(), g.number_of_dst_nodes(), g.number_of_edges()
    Bc = R if B is None else B
    glim = min(lim, 2) if Fw >= 256 else lim
    f = lambda m, *s: torch.from_numpy(rng.integers(-m, m + 1, s).astype(np.float32))
    case = dict(x=f(lim, n_src, Fw), y=f(lim, n_src, Bc, Fw), dZ=f(glim, n_dst, Bc, Fw), dout=f(glim, n_dst, Fw),
                coef=None if B is None else f(8, R, B) * 0.25, norm=torch.from_numpy(rng.choice(np.array([0.25, 0.5, 1.0, 2.0], dtype=np.float32), E)),
                et=relations(g, R, seed + 1))
    ref = reference(g, case, absolute=True)
    for name, quantum in (("Z", 2.0 ** -4), ("out", 2.0 ** -4), ("dx", 2.0 ** -4), ("dy", 2.0 ** -4), ("dcoef_e", 2.0 ** -2), ("dcoef_c", 2.0 ** -2)):
        t = ref[name]
        assert t.numel() == 0 or float(t.max()) < min(2.0 ** 24 * quantum, 2.0 ** 22), (name, float(t.max()))
    return case


def reference(g, case, absolute=False, norm=True, mistake=None):
    """Everything the two ops compute on `case`, in float64 from the formulas -> dict(Z, out, dx, dy, dcoef_e, dcoef_c), or - absolute - the
    sums of the absolute terms.  `mistake`: one of the three planted ones the bounds must catch ("drop": the last in-edge of the longest
    row is left out; "relation": one edge's relation replaced by another; "coef": a relative error of 1e-5 on the coefficients)."""
    src, dst, n_src, n_dst = edge_lists(g)
    R = int(case["coef"].shape[0]) if case["coef"] is not None else int(case["y"].shape[1])
    et = case["et"].clone()
    c = case["norm"].double() if norm else torch.ones(src.numel(), dtype=F64)
    coef = full_coef(case["coef"], R)
    if mistake == "drop":
        row = int(torch.argmax(torch.bincount(dst, minlength=n_dst)))
        c = c.clone()
        c[int(position_last_edge(g, row))] = 0.0
    elif mistake == "relation":
        e = int(torch.nonzero(dst == int(torch.argmax(torch.bincount(dst, minlength=n_dst))))[0])
        et[e] = (et[e] + 1) % max(R - 1, 2) if R > 1 else et[e]
    elif mistake == "coef":
        coef = coef * (1.0 + 1e-5)
    x, y, dZ, dout = (case[k].double() for k in ("x", "y", "dZ", "dout"))
    dx, dce = expand_grads64(src, dst, et, c, coef, x, dZ, absolute)
    dy, dcc = contract_grads64(src, dst, et, c, coef, y, dout, absolute)
    return dict(Z=expand64(src, dst, et, c, coef, x, n_dst, absolute), out=contract64(src, dst, et, c, coef, y, n_dst, absolute), dx=dx, dy=dy,
                dcoef_e=dce, dcoef_c=dcc)


def position_last_edge(g, row):
    """The edge id at the last CSC position of `row`."""
    return g.csc.eid.cpu().long()[int(g.csc.indptr[row + 1]) - 1]


def bounds(g, case, norm=True):
    """The derived rounding bounds (module docstring) of everything in `reference`."""
    src, dst, n_src, n_dst = edge_lists(g)
    a = reference(g, case, absolute=True, norm=norm)
    onehot = case["coef"] is None
    R = int(case["y"].shape[1]) if onehot else int(case["coef"].shape[0])
    B, Fw = (1 if onehot else int(case["coef"].shape[1])), int(case["x"].shape[1])
    c_in = c_out = g.csc.chunk                                                  # both directions of a graph are planned with one chunk
    ex_in, ex_out = expand_factor(dst, n_dst, c_in), expand_factor(src, n_src, c_out)
    co_in, co_out = contract_factor(dst, n_dst, c_in, B), contract_factor(src, n_src, c_out, B)
    dc = dcoef_factor(case["et"], R, Fw).view(-1, 1)
    return dict(Z=ex_in.view(-1, 1, 1) * a["Z"], out=co_in.view(-1, 1) * a["out"], dx=co_out.view(-1, 1) * a["dx"],
                dy=ex_out.view(-1, 1, 1) * a["dy"], dcoef_e=dc * a["dcoef_e"], dcoef_c=dc * a["dcoef_c"])


def run_ops(g, case, dev, impl=None, norm=True):
    """`ops.rel_expand_sum` and `ops.rel_contract_sum` with their gradients on `case` -> the dict of `reference` as float64 CPU tensors
    (dcoef_* absent in one-hot mode)."""
    from bot_amd import ops
    R = int(case["y"].shape[1]) if case["coef"] is None else int(case["coef"].shape[0])
    et, nm = case["et"].to(dev), (case["norm"].to(dev) if norm else None)
    got = {}
    for op, inp, up, names in ((ops.rel_expand_sum, "x", "dZ", ("Z", "dx", "dcoef_e")), (ops.rel_contract_sum, "y", "dout", ("out", "dy", "dcoef_c"))):
        t = case[inp].clone().to(dev).requires_grad_()
        coef = None if case["coef"] is None else case["coef"].clone().to(dev).requires_grad_()
        res = op(g, t, et, R, coef, nm, impl=impl)
        assert res.dtype == torch.float32 and tuple(res.shape) == tuple(case[up].shape)
        res.backward(case[up].to(dev))
        got[names[0]], got[names[1]] = res.detach().cpu().double(), t.grad.cpu().double()
        if coef is not None:
            got[names[2]] = coef.grad.cpu().double()
    return got


def record(worst, name, err, lim):
    frac = float((err / lim.clamp(min=1e-300)).max()) if err.numel() else 0.0
    if worst is not None:
        worst[name] = max(worst.get(name, 0.0), frac)
    return frac


def check_bounds(g, case, dev, impl, worst=None, norm=True):
    """Both sweeps over the CSC, their gradients over the CSR and dcoef on `case` against float64 under the derived bounds."""
    got = run_ops(g, case, dev, impl, norm)
    want, lim = reference(g, case, norm=norm), bounds(g, case, norm)
    for name, x in got.items():
        err = (x - want[name]).abs()
        frac = record(worst, f"{impl or 'default'} {name}", err, lim[name])
        assert bool((err <= lim[name]).all()), (impl, name, tuple(x.shape), frac)
    return got


def check_exact(g, case, dev, impl=None):
    """The same on an exact-regime case: every entry equals the float64 restatement."""
    got = run_ops(g, case, dev, impl)
    want = reference(g, case)
    for name, x in got.items():
        assert np.array_equal(x.numpy(), want[name].numpy()), (impl, name, tuple(x.shape))
    return got


# ------------------------------------------------------------------------------------------------ layer and stack, float64 torch
def relconv64(conv, src, dst, n_dst, et, c, h_src, h_dst, p):
    """`RelGraphConv` (dropout 0) in float64: per relation the weighted sum of the sources' rows times W_r = sum_b w_comp[r, b] V_b (V_r
    without w_comp); p: the layer's parameters as float64 tensors keyed like its named_parameters; c float64 [E] or None."""
    V = p["weight"]
    out = torch.zeros((n_dst, V.shape[2]), dtype=F64)
    for r in range(conv.num_rels):
        m = et == r
        if not bool(m.any()):
            continue
        W = torch.einsum("b,bio->io", p["w_comp"][r], V) if "w_comp" in p else V[r]
        msg = h_src[src[m]] if c is None else h_src[src[m]] * c[m].unsqueeze(1)
        out = out + torch.zeros((n_dst, h_src.shape[1]), dtype=F64).index_add(0, dst[m], msg) @ W
    if "h_bias" in p:
        out = out + p["h_bias"]
    if "loop_weight" in p:
        out = out + h_dst @ p["loop_weight"]
    if conv.layer_norm:
        out = torch.nn.functional.layer_norm(out, (out.shape[1],), p["layer_norm_weight.weight"], p["layer_norm_weight.bias"], conv.layer_norm_weight.eps)
    return out if conv.activation is None else conv.activation(out)


def rgcn_stack64(model, layers, feat, p):
    """`RGCN` in eval mode (no dropout, BatchNorm by its running statistics) in float64; layers: per layer (src, dst, n_dst, et, c)."""
    h = feat
    n = len(model.convs)
    for i, (src, dst, n_dst, et, c) in enumerate(layers):
        h = relconv64(model.convs[i], src, dst, n_dst, et, c, h, h[:n_dst], layer_params(p, i))
        if i < n - 1:
            if len(model.norms):
                bn = model.norms[i]
                h = (h - bn.running_mean.cpu().double()) * torch.rsqrt(bn.running_var.cpu().double() + bn.eps) * p[f"norms.{i}.weight"] + p[f"norms.{i}.bias"]
            h = torch.relu(h)
    return h


def make_conv(fin, fout, R, seed, **kw):
    """A RelGraphConv with seeded weights and a non-zero bias."""
    from bot_amd import nn as bnn
    torch.manual_seed(seed)
    conv = bnn.RelGraphConv(fin, fout, R, **kw)
    if conv.h_bias is not None:
        with torch.no_grad():
            conv.h_bias.copy_(torch.randn(conv.h_bias.shape, generator=torch.Generator().manual_seed(seed + 100)))
    return conv


def check_conv(g, dev, fin, fout, R, seed=0, pair=False, with_norm=True, order=None, **kw):
    """One `RelGraphConv` forward + backward on `g` against `relconv64` under the suite's own criteria (tests/parity_cases.py): the
    output, and the gradients of the input(s) and of every parameter.  pair: the layer takes a (feat_src, feat_dst) pair."""
    from tests.parity_cases import fwd_close, grad_close
    src, dst, n_src, n_dst = edge_lists(g)
    conv = make_conv(fin, fout, R, seed, **kw).to(dev)
    conv.order = order
    gen = torch.Generator().manual_seed(seed + 1)
    x_src = torch.randn(n_src, fin, generator=gen)
    x_dst = torch.randn(n_dst, fin, generator=gen) if pair else None
    dout = torch.randn(n_dst, fout, generator=gen)
    et = relations(g, R, seed + 2)
    nm = (torch.rand(src.numel(), 1, generator=gen) + 0.25) if with_norm else None
    xs = x_src.clone().to(dev).requires_grad_()
    xd = None if x_dst is None else x_dst.clone().to(dev).requires_grad_()
    out = conv(g, (xs, xd) if pair else xs, et.to(dev), None if nm is None else nm.to(dev))
    assert out.shape == (n_dst, fout)
    out.backward(dout.to(dev))
    p = params64(conv)
    s64 = x_src.double().requires_grad_()
    d64 = None if x_dst is None else x_dst.double().requires_grad_()
    ref = relconv64(conv, src, dst, n_dst, et, None if nm is None else nm.double().view(-1), s64, s64[:n_dst] if d64 is None else d64, p)
    ref.backward(dout.double())
    fwd_close(out, ref.detach().numpy())
    grad_close(xs.grad, s64.grad.numpy())
    if pair:
        grad_close(xd.grad, d64.grad.numpy())
    for name, prm in conv.named_parameters():
        grad_close(prm.grad, p[name].grad.numpy())
    return conv, out.detach()


def check_stack(model, graphs, feat, dev):
    """`RGCN` in eval mode on a Graph or a block list, relations and norm from edata["etype"] / edata["norm"], against `rgcn_stack64`:
    output, input gradient and every parameter's gradient."""
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
    layers = [edge_lists(g)[:2] + (g.number_of_dst_nodes(), g.edata["etype"].cpu().long(), g.edata["norm"].cpu().double().view(-1)) for g in per_layer]
    ref = rgcn_stack64(model, layers, f64, p)
    ref.backward(dout.double())
    fwd_close(out, ref.detach().numpy())
    grad_close(x.grad, f64.grad.numpy())
    for name, prm in model.named_parameters():
        grad_close(prm.grad, p[name].grad.numpy())
