"""Float64 restatement of the contract of bot_amd/smoothing.py (label propagation, Correct and Smooth) and of one
`bot_propagate_step_f32` sweep, in plain torch ops on the CPU; the fixtures the host and the GPU tests share.  Nothing here imports the
package under test."""
import functools
import math

import torch

F64 = torch.float64
INF = math.inf
POSTS = {"clamp01": (0.0, 1.0), "clamp11": (-1.0, 1.0), None: (-INF, INF)}


# ------------------------------------------------------------------------------------------------ graphs
def powerlaw_graph(n, e, seed, n_isolated=3):
    """Directed power-law multigraph (endpoints floor(n u^2), ids relabelled at random) in which `n_isolated` nodes touch no edge at
    all; many more have no in-edge.  (src, dst) int64."""
    gen = torch.Generator().manual_seed(seed)
    src = (n * torch.rand(e, generator=gen, dtype=F64) ** 2).long().clamp_(max=n - 1)
    dst = (n * torch.rand(e, generator=gen, dtype=F64) ** 2).long().clamp_(max=n - 1)
    perm = torch.randperm(n, generator=gen)
    src, dst = perm[src], perm[dst]
    lonely = torch.randperm(n, generator=gen)[:min(n_isolated, max(n - 1, 0))]
    keep = ~(torch.isin(src, lonely) | torch.isin(dst, lonely))
    return src[keep].contiguous(), dst[keep].contiguous()


def planted_graph(n, k, e, p_in, seed):
    """Undirected graph with k planted communities (node i in community i % k): an edge's second endpoint lies in the first one's
    community with probability p_in.  (src, dst, community)."""
    gen = torch.Generator().manual_seed(seed)
    a = torch.randint(0, n, (e,), generator=gen)
    inside = torch.rand(e, generator=gen) < p_in
    same = (torch.randint(0, n // k, (e,), generator=gen) * k + a % k).clamp_(max=n - 1)
    b = torch.where(inside, same, torch.randint(0, n, (e,), generator=gen))
    return torch.cat([a, b]), torch.cat([b, a]), torch.arange(n) % k


# ------------------------------------------------------------------------------------------------ the contract
def scales(dst, n, adj):
    """(src_scale, dst_scale) float64 [n] or None: P y = dst_scale * A (src_scale * y)."""
    deg = torch.bincount(dst, minlength=n).to(F64).clamp(min=1)
    return {"DAD": (deg ** -0.5, deg ** -0.5), "DA": (None, 1.0 / deg), "AD": (1.0 / deg, None)}[adj]


def step(src, dst, y, y0, alpha, beta, src_scale, dst_scale, lo, hi, fixed=None):
    """One sweep in float64: (out, row_abs, bound) with `bound` the sum over the in-edges of |src_scale y| (what a rounding bound of
    the row's sum is relative to)."""
    y, y0 = y.to(F64), y0.to(F64)
    t = y if src_scale is None else y * src_scale.to(F64)[:, None]
    s = torch.zeros_like(y0).index_add_(0, dst, t[src])
    mag = torch.zeros_like(y0).index_add_(0, dst, t[src].abs())
    if dst_scale is not None:
        s, mag = s * dst_scale.to(F64)[:, None], mag * dst_scale.to(F64)[:, None]
    out = (alpha * s + beta * y0).clamp(lo, hi)
    if fixed is not None:
        out = torch.where(fixed.bool()[:, None], y0, out)
    return out, out.abs().sum(1), abs(alpha) * mag + abs(beta) * y0.abs()


def member(n, mask):
    mask = torch.as_tensor(mask)
    if mask.dtype == torch.bool:
        return mask
    m = torch.zeros(n, dtype=torch.bool)
    m[mask] = True
    return m


def propagate(src, dst, n, y_start, num_layers, alpha, adj, post_step):
    """y <- post(alpha P y + (1 - alpha) y_start), num_layers times, float64."""
    ss, ds = scales(dst, n, adj)
    if isinstance(post_step, tuple):
        lo, hi, fixed = -INF, INF, member(n, post_step[0])
    else:
        (lo, hi), fixed = POSTS[post_step], None
    y0 = y_start.to(F64)
    y = y0
    for _ in range(num_layers):
        y = step(src, dst, y, y0, alpha, 1.0 - alpha, ss, ds, lo, hi, fixed)[0]
    return y


def onehot(labels, C):
    return torch.zeros((labels.numel(), C), dtype=F64).scatter_(1, labels.reshape(-1, 1).long(), 1.0)


def label_propagation(src, dst, n, labels, num_layers, alpha, adj="DAD", mask=None, post_step="clamp01"):
    y = labels.to(F64) if labels.is_floating_point() else onehot(labels, int(labels.max()) + 1)
    if mask is not None:
        y = torch.where(member(n, mask)[:, None], y, torch.zeros((), dtype=F64))
    return propagate(src, dst, n, y, num_layers, alpha, adj, post_step)


def _index(n, mask):
    mask = torch.as_tensor(mask)
    return torch.nonzero(mask).squeeze(1) if mask.dtype == torch.bool else mask.long()


def correct(src, dst, n, y_soft, y_true, mask, num_layers=50, alpha=0.8, adj="DAD", autoscale=True, scale=1.0):
    """(corrected float64 [n, C], raw autoscale factors float64 [n] before the `> 1000 -> 1` rule, or None)."""
    idx = _index(n, mask)
    y_soft = y_soft.to(F64)
    E = torch.zeros_like(y_soft)
    E[idx] = onehot(y_true, y_soft.shape[1]) - y_soft[idx]
    if autoscale:
        Eh = propagate(src, dst, n, E, num_layers, alpha, adj, "clamp11")
        sigma = E[idx].abs().sum() / idx.numel()
        raw = sigma / Eh.abs().sum(1)
        s = torch.where(torch.isinf(raw) | (raw > 1000.0), torch.ones((), dtype=F64), raw)
        out = y_soft + s[:, None] * Eh
    else:
        raw = None
        out = y_soft + scale * propagate(src, dst, n, E, num_layers, alpha, adj, (idx, "fix"))
    return torch.where(torch.isfinite(out), out, y_soft), raw


def smooth(src, dst, n, y_soft, y_true, mask, num_layers=50, alpha=0.8, adj="DAD"):
    idx = _index(n, mask)
    y = y_soft.to(F64).clone()
    y[idx] = onehot(y_true, y.shape[1])
    return propagate(src, dst, n, y, num_layers, alpha, adj, "clamp01")


def correct_and_smooth(src, dst, n, y_soft, y_true, mask, num_layers=50, alpha=0.8, adj="DAD", autoscale=True, scale=1.0):
    """The same layers / alpha / adj for both stages.  (smoothed, raw autoscale factors or None)."""
    c, raw = correct(src, dst, n, y_soft, y_true, mask, num_layers, alpha, adj, autoscale, scale)
    return smooth(src, dst, n, c, y_true, mask, num_layers, alpha, adj), raw


def scale_margin(raw):
    """Smallest relative distance of a finite raw autoscale factor from the threshold 1000 (inf when there is none): the rule
    `> 1000 -> 1` is a discontinuity, a comparison across it means nothing."""
    if raw is None:
        return INF
    fin = raw[torch.isfinite(raw)]
    return float(((fin - 1000.0).abs() / 1000.0).min()) if fin.numel() else INF


# ------------------------------------------------------------------------------------------------ an independent dense formulation
def dense_P(src, dst, n, adj):
    A = torch.zeros((n, n), dtype=F64)
    A.index_put_((dst, src), torch.ones(src.numel(), dtype=F64), accumulate=True)          # A[v, u] = number of edges u -> v
    d = A.sum(1).clamp(min=1)
    if adj == "DAD":
        return torch.diag(d ** -0.5) @ A @ torch.diag(d ** -0.5)
    return torch.diag(1.0 / d) @ A if adj == "DA" else A @ torch.diag(1.0 / d)


def dense_propagate(P, y_start, num_layers, alpha, lo, hi, fixed_idx=None):
    y0 = y_start.to(F64)
    y = y0
    for _ in range(num_layers):
        y = (alpha * (P @ y) + (1.0 - alpha) * y0).clamp(lo, hi)
        if fixed_idx is not None:
            y[fixed_idx] = y0[fixed_idx]
    return y


# ------------------------------------------------------------------------------------------------ shared fixtures
# (nodes, edges, seed); the seeds are those for which no row's raw autoscale factor lies within 1 % of 1000 for any of the cases
# the tests run (checked by every test that compares across the rule, before it compares)
GRAPHS = {"small": (3000, 12000, 6), "large": (20000, 137000, 9), "tiny": (300, 1500, 3)}


@functools.lru_cache(maxsize=None)
def graph(name):
    n, e, seed = GRAPHS[name]
    src, dst = powerlaw_graph(n, e, seed)
    return src, dst, n


@functools.lru_cache(maxsize=None)
def cs_inputs(name, C, seed=0):
    """(y_soft float32 [n, C] = a softmax, y_true int64 [m], mask int64 [m]): 30 % of the nodes labelled, in random order."""
    n = GRAPHS[name][0]
    gen = torch.Generator().manual_seed(1000 * seed + 17 * C + n)
    y_soft = torch.softmax(2.0 * torch.randn(n, C, generator=gen), dim=-1)
    labels = torch.randint(0, C, (n,), generator=gen)
    mask = torch.randperm(n, generator=gen)[: max(1, int(0.3 * n))]
    return y_soft, labels[mask].contiguous(), mask.contiguous()


@functools.lru_cache(maxsize=None)
def cs_reference(name, C, adj, autoscale, alpha=0.8, num_layers=50):
    """The float64 result of the full Correct and Smooth run on a fixture, computed once per session: (smoothed, raw factors)."""
    src, dst, n = graph(name)
    y_soft, y_true, mask = cs_inputs(name, C)
    return correct_and_smooth(src, dst, n, y_soft, y_true, mask, num_layers, alpha, adj, autoscale)


@functools.lru_cache(maxsize=None)
def lp_reference(name, C, adj, alpha=0.8, num_layers=50):
    src, dst, n = graph(name)
    _, y_true, mask = cs_inputs(name, C)
    labels = torch.zeros(n, dtype=torch.int64)
    labels[mask] = y_true
    labels[0] = C - 1                                  # the one-hot width is labels.max() + 1
    return labels, label_propagation(src, dst, n, labels, num_layers, alpha, adj, mask=mask)
