"""Personalised-PageRank propagation that can be trained through (`ops.appnp_propagate`): the core of APPNP (Gasteiger, Bojchevski,
Günnemann, ICLR 2019; DGL's `APPNPConv`) and of GCNII (Chen et al., ICML 2020; DGL's `GCN2Conv`).

    h_0 = x;   h_t = (1 - alpha) * P_t h_{t-1} + alpha * h0   (t = 1..k),   P_t = D_dst (A o M_t) D_src

with the degree scales of `smoothing._degree_scales` (in-degree, clamp(min=1); with an edge weight the weighted in-degree) and M_t the
edge-drop mask of step t over CSC positions, rescaled by 1 / (1 - p): position q is kept iff word q & 3 of Philox4x32-10 under the key
`seed` at the counter (t << 32) | (q >> 2), shifted right by 8 and times 2^-24, is >= p (`appnp_keep`).

impl="kernel": one `bot_appnp_step_f32` launch per step and direction (csrc/appnp.hip).  The propagation is linear in h, so the backward

    g_k = dout;   g_{t-1} = (1 - alpha) * P_t^T g_t;   dx = g_0;   dh0 = alpha * sum_{t=1..k} g_t   (summed into dx when h0 is x)

needs no activation, and the kernel regenerates each step's mask from (seed, t): the autograd node saves NO tensor - a seed.  P_t^T is
the same entry point over the CSR with the two scales swapped and pos = csr2csc; the sum for dh0 rides in the sweeps' epilogue
(acc_out = acc_in + o), the sweep for t = 1 adds alpha * acc through y0, so the backward is k launches and no extra pass.  Between the
sweeps of a direction the iterate stays multiplied by the next sweep's source scale (out_scale), as in `smoothing._propagate_kernel`.
impl="tensor": the same function of the same seed in tensor ops - on the GPU `ops.u_mul_e_sum` with the step's factors as position-order
weights and alpha * h0 as addend, on the CPU gather / `index_add_` - which keeps k matrices [N, C] and k weight vectors [E] for its
backward.  It is what runs on CPU tensors and what the kernel form is timed against (tools/bench_appnp.py)."""
from __future__ import annotations

import os

import torch

from . import smoothing

__all__ = ["appnp_keep", "appnp_propagate", "propagate_scaled", "default_impl"]

_M32 = 0xFFFFFFFF

# impl=None takes the kernel form on the GPU only at the settings where it beat the tensor form by more than that form's round-to-round
# spread (tools/bench_appnp.py, README "APPNP and GCNII"); the measurement sets these flags.
KERNEL_DEFAULT = {"plain": True, "drop": True}


def default_impl(x, edge_drop=0.0) -> str:
    """"tensor" for CPU tensors; on the GPU "kernel" unless BOT_APPNP=tensor or the setting's `KERNEL_DEFAULT` flag is off."""
    if not x.is_cuda or os.environ.get("BOT_APPNP", "").lower() == "tensor":
        return "tensor"
    return "kernel" if KERNEL_DEFAULT["drop" if edge_drop > 0 else "plain"] else "tensor"


def _mulhilo(m: int, c):
    """(high, low) 32-bit words of m * c for a 32-bit constant m and int64 tensors c in [0, 2^32), without leaving int64's range."""
    a, b = m * (c >> 16), m * (c & 0xFFFF)           # both below 2^48
    return (a + (b >> 16)) >> 16, (((a & 0xFFFF) << 16) + b) & _M32


def _philox4x32_10(seed: int, c0, c1: int):
    """Philox4x32-10 (csrc/common.h Philox::gen) in int64 tensor arithmetic: key `seed` (64 bits), counters (c0 tensor, c1 scalar, 0, 0)
    -> int64 [n, 4] of 32-bit words.  Valid on CPU and GPU tensors."""
    k0, k1 = seed & _M32, (seed >> 32) & _M32
    c1 = torch.full_like(c0, c1 & _M32)
    c2, c3 = torch.zeros_like(c0), torch.zeros_like(c0)
    for _ in range(10):
        h0, l0 = _mulhilo(0xD2511F53, c0)
        h1, l1 = _mulhilo(0xCD9E8D57, c2)
        c0, c1, c2, c3 = h1 ^ c1 ^ k0, l1, h0 ^ c3 ^ k1, l0
        k0, k1 = (k0 + 0x9E3779B9) & _M32, (k1 + 0xBB67AE85) & _M32
    return torch.stack([c0, c1, c2, c3], dim=1)


def appnp_keep(seed, step, E, p, device="cpu"):
    """bool [E] over CSC positions: the positions edge dropout at rate `p` KEEPS at step `step` under `seed` - bit for bit the mask
    csrc/appnp.hip regenerates (module docstring)."""
    E, seed = int(E), int(seed) & 0xFFFFFFFFFFFFFFFF
    n4 = (E + 3) // 4
    words = _philox4x32_10(seed, torch.arange(n4, dtype=torch.int64, device=device), int(step)).reshape(-1)[:E]
    u = (words >> 8).to(torch.float32) * (1.0 / 16777216.0)
    return u >= torch.tensor(float(p), dtype=torch.float32, device=device)


def _csr_weights(g, ws):
    """The edge weights in CSR position order (what the backward sweep streams), cached beside the CSC-order copy."""
    if ws is None:
        return None
    if "csr" not in ws:
        ws["csr"] = ws["pos"][g.csr2csc.long()].contiguous()
    return ws["csr"]


def _forward_kernel(g, x, h0, k, alpha, src_scale, dst_scale, p, seed, ws):
    from . import _C
    d = g.csc
    start = x.contiguous()
    h0 = start if h0 is None else h0.contiguous()
    C = start.shape[1]
    ew = None if ws is None else ws["pos"]
    bufs = (torch.empty_like(start), torch.empty_like(start) if k > 1 else None)
    partial = torch.empty(d.n_slots * C, dtype=torch.float32, device=x.device) if d.n_long else None
    y = start
    for t in range(1, k + 1):
        out = bufs[(t - 1) & 1]
        # between sweeps the iterate stays multiplied by the source scale (out_scale): only the first sweep reads src_scale per edge
        _C.appnp_step(d, y, out, 1.0 - alpha, alpha, y0=h0, src_scale=src_scale if t == 1 else None, dst_scale=dst_scale,
                      out_scale=None if t == k else src_scale, ew=ew, p=p, seed=seed, step=t, partial=partial)
        y = out
    return y


def _backward_kernel(g, dout, k, alpha, src_scale, dst_scale, p, seed, ws, shared, want_dx=True):
    """(dx, dh0): dh0 None when h0 is x (its part is inside dx)."""
    from . import _C
    d = g.csr
    gk = dout.contiguous()
    C = gk.shape[1]
    ew = _csr_weights(g, ws)
    pos = g.csr2csc if p > 0 else None                   # the mask's index of a CSR position: the forward's CSC position
    S, D = dst_scale, src_scale                            # P^T = D_src A^T D_dst: the two scales swap roles
    partial = torch.empty(d.n_slots * C, dtype=torch.float32, device=gk.device) if d.n_long else None
    bufs = (torch.empty_like(gk), torch.empty_like(gk) if k > 2 else None)
    acc, y, i = None, gk, 0
    for t in range(k, 1, -1):                              # g_{t-1} and acc += g_{t-1}; acc starts as dout
        first = t == k
        if first:
            acc = torch.empty_like(gk)
        _C.appnp_step(d, y, bufs[i], 1.0 - alpha, 0.0, src_scale=S if first else None, dst_scale=D, out_scale=S, acc_in=gk if first else acc,
                      acc_out=acc, ew=ew, pos=pos, p=p, seed=seed, step=t, partial=partial)
        y, i = bufs[i], i ^ 1
    total = gk if acc is None else acc                     # sum_{t=1..k} g_t
    dx = None
    if want_dx or shared:
        dx = bufs[i] if bufs[i] is not None else torch.empty_like(gk)
        _C.appnp_step(d, y, dx, 1.0 - alpha, alpha, y0=total if shared else None, src_scale=S if k == 1 else None, dst_scale=D, ew=ew,
                      pos=pos, p=p, seed=seed, step=1, partial=partial)
    return dx, (None if shared else alpha * total)


class _AppnpKernel(torch.autograd.Function):
    """The kernel form: nothing is saved for the backward but the graph and the seed."""

    @staticmethod
    def forward(ctx, g, x, h0, k, alpha, adj, p, seed, ws):
        scales = smoothing._degree_scales(g, adj, ws)
        ctx.g, ctx.k, ctx.alpha, ctx.p, ctx.seed, ctx.ws, ctx.scales, ctx.shared = g, k, alpha, p, seed, ws, scales, h0 is None
        return _forward_kernel(g, x, h0, k, alpha, scales[0], scales[1], p, seed, ws)

    @staticmethod
    def backward(ctx, dout):
        dx, dh0 = _backward_kernel(ctx.g, dout, ctx.k, ctx.alpha, ctx.scales[0], ctx.scales[1], ctx.p, ctx.seed, ctx.ws, ctx.shared,
                                   want_dx=ctx.needs_input_grad[1])
        return None, dx, dh0, None, None, None, None, None, None


class _ScaledP(torch.autograd.Function):
    """a * P x on the kernel: one sweep without y0 forward, one over the CSR backward; nothing is saved."""

    @staticmethod
    def forward(ctx, g, x, a, adj, ws):
        from . import _C
        ss, ds = smoothing._degree_scales(g, adj, ws)
        ctx.g, ctx.a, ctx.ws, ctx.scales = g, a, ws, (ss, ds)
        x = x.contiguous()
        return _C.appnp_step(g.csc, x, torch.empty_like(x), a, src_scale=ss, dst_scale=ds, ew=None if ws is None else ws["pos"])

    @staticmethod
    def backward(ctx, dout):
        from . import _C
        ss, ds = ctx.scales
        d = dout.contiguous()
        return None, _C.appnp_step(ctx.g.csr, d, torch.empty_like(d), ctx.a, src_scale=ds, dst_scale=ss, ew=_csr_weights(ctx.g, ctx.ws)), None, None, None


def propagate_scaled(g, x, a, *, adj="DAD", edge_weight=None, impl=None):
    """a * P x with `appnp_propagate`'s P, graphs, edge weights and impl rule (no edge dropout, no h0 term): GCN2Conv's propagation when the
    initial features take a projection of their own."""
    y0 = torch.zeros((), dtype=x.dtype, device=x.device).expand_as(x)
    impl = default_impl(x) if impl is None else impl
    if impl == "tensor":
        return appnp_propagate(g, x, 1, 1.0 - float(a), h0=y0, adj=adj, edge_weight=edge_weight, impl="tensor")
    appnp_propagate(g, x, 0, 0.0, adj=adj, edge_weight=edge_weight, impl="kernel")            # the argument checks
    ws = smoothing._weights(g, edge_weight)
    C = x.shape[1]
    Cp = C if (C % 4 == 0 or C < 5) else C + 4 - C % 4
    y = _ScaledP.apply(g, x if Cp == C else torch.nn.functional.pad(x, (0, Cp - C)), float(a), adj, ws)
    return y if Cp == C else y[:, :C].contiguous()


def _csc_rows(g):
    """int64 [E]: the destination row of every CSC position, cached per graph."""
    c = smoothing._cache(g)
    if "csc_rows" not in c:
        d = g.csc
        c["csc_rows"] = torch.repeat_interleave(torch.arange(d.n_rows, device=d.indptr.device), (d.indptr[1:] - d.indptr[:-1]).long(),
                                                output_size=d.nnz)
    return c["csc_rows"]


def _tensor(g, x, h0, k, alpha, adj, p, seed, ws):
    h0 = x if h0 is None else h0
    E = g.number_of_edges()
    factor = lambda t: appnp_keep(seed, t, E, p, x.device).to(torch.float32) * (1.0 / (1.0 - p))
    h = x
    if x.is_cuda:
        from . import ops
        base = (1.0 - alpha) * smoothing._edge_weights(g, adj, ws)
        addend = alpha * h0
        for t in range(1, k + 1):
            w = base if p == 0 else base * factor(t).view(-1, 1)
            h = ops.u_mul_e_sum(g, h, w, order="csc", addend=addend)
        return h
    src_scale, dst_scale = smoothing._degree_scales(g, adj, ws)
    src, dst = g.csc.indices.long(), _csc_rows(g)
    we = None if ws is None else ws["pos"]
    for t in range(1, k + 1):
        f = we
        if p > 0:
            f = factor(t) if f is None else f * factor(t)
        m = (h if src_scale is None else h * src_scale[:, None])[src]
        s = torch.zeros_like(h).index_add_(0, dst, m if f is None else m * f[:, None])
        if dst_scale is not None:
            s = s * dst_scale[:, None]
        h = (1.0 - alpha) * s + alpha * h0
    return h


def appnp_propagate(g, x, k, alpha, *, h0=None, adj="DAD", edge_drop=0.0, seed=None, edge_weight=None, impl=None):
    """h_k of h_0 = x, h_t = (1 - alpha) * P_t h_{t-1} + alpha * h0 (module docstring); differentiable in x and h0.
    x, h0: float32 [N, C] on g's device in the graph's own node numbering; `h0`: x when None.  `edge_drop`: the rate of the per-step edge
    dropout (the caller zeroes it in eval mode); `seed`: of its Philox stream, drawn with `ops.new_dropout_seed` when None.
    `edge_weight`: float32 [E] / [E, 1] in edge-id order or an edata key, constant (one that requires a gradient raises ValueError): the
    weighted in-degree replaces the degree.  Whole graphs and `Subgraph`s; a block or a partition with a halo raises ValueError.
    impl: "kernel", "tensor" or None (`default_impl`)."""
    smoothing._square(g)
    if adj not in smoothing._ADJ:
        raise ValueError(f"adj={adj!r}: one of {smoothing._ADJ}")
    k, alpha, p = int(k), float(alpha), float(edge_drop)
    if k < 0:
        raise ValueError("k must be >= 0")
    if not 0.0 <= p < 1.0:
        raise ValueError(f"edge_drop={edge_drop!r}: a rate in [0, 1)")
    n = g.number_of_nodes()
    shared = h0 is None or h0 is x
    for t, name in ((x, "x"),) + (() if shared else ((h0, "h0"),)):
        if t.dim() != 2 or t.shape[0] != n or t.dtype != torch.float32:
            raise ValueError(f"{name} must be float32 [{n}, C], got {tuple(t.shape)} {t.dtype}")
        if t.device != g.device:
            raise ValueError(f"{name} lives on {t.device}, the graph on {g.device}")
    if not shared and h0.shape != x.shape:
        raise ValueError(f"h0 must have x's shape {tuple(x.shape)}, got {tuple(h0.shape)}")
    w = g.edata[edge_weight] if isinstance(edge_weight, str) else edge_weight
    if isinstance(w, torch.Tensor) and w.requires_grad:
        raise ValueError("appnp_propagate has no gradient for edge_weight (DESIGN §8): pass a constant weight (detach it)")
    ws = smoothing._weights(g, edge_weight)
    impl = default_impl(x, p) if impl is None else impl
    if impl not in ("kernel", "tensor"):
        raise ValueError(f"impl={impl!r}: 'kernel' or 'tensor'")
    if k == 0:
        return x
    if seed is None:
        from . import ops
        seed = ops.new_dropout_seed(p)
    seed = int(seed)
    C = x.shape[1]
    # odd widths run padded with zero columns on the GPU (smoothing.propagate's rule); they stay zero in both directions
    Cp = C if (not x.is_cuda or C % 4 == 0 or C < 5) else C + 4 - C % 4
    if Cp != C:
        x = torch.nn.functional.pad(x, (0, Cp - C))
        h0 = None if shared else torch.nn.functional.pad(h0, (0, Cp - C))
    h0 = None if shared else h0
    if impl == "kernel":
        y = _AppnpKernel.apply(g, x, h0, k, alpha, adj, p, seed, ws)
    else:
        y = _tensor(g, x, h0, k, alpha, adj, p, seed, ws)
    return y if Cp == C else y[:, :C].contiguous()
