"""Numpy / float64 restatements of the GraphSAGE contracts (include/bot_gnn.h "Max aggregation"), shared by
tests/test_sage_host.py and tests/test_sage_gpu.py: the max sweep with its tie, empty-row and relu rules, its backward, the three
`SAGEConv` aggregators and the `GraphSAGE` stack; and CPU stand-ins for `_C.spmm_max` / `_C.spmm_max_bwd`, which the host suite
monkeypatches beside `tests._oracle_backend.install`.  The restatements call nothing of the code under test; the `check_*` functions at the
end run a layer or a stack against them, on whatever device the graph lives on (both suites share them)."""
import numpy as np
import torch

F64 = torch.float64


# ------------------------------------------------------------------------------------------------ the max sweep
def max_forward(indptr, indices, x, relu=False):
    """(out, arg) of one direction: out[r, f] = max_k x[indices[k], f] over the positions k of row r, arg[r, f] the SMALLEST such k
    (numeric ties: -0.0 == +0.0); an empty row is (0, -1); relu: out = max(m, 0) and arg = -1 wherever m <= 0.  x keeps its dtype:
    a max does not round."""
    indptr, indices = np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64)
    n, F = len(indptr) - 1, x.shape[1]
    out = np.zeros((n, F), dtype=x.dtype)
    arg = np.full((n, F), -1, dtype=np.int32)
    for r in range(n):
        b, e = indptr[r], indptr[r + 1]
        if e == b:
            continue
        seg = x[indices[b:e]]
        m = seg.max(0)
        out[r] = m
        arg[r] = b + np.argmax(seg == m, axis=0)       # the first position that attains the max
    if relu:
        gate = ~(out > 0)
        out[gate] = 0
        arg[gate] = -1
    return out, arg


def max_backward(indices, n_src, dout, arg):
    """dx[u, f] = the sum of dout[r, f] over the (r, f) whose arg names a position of source u; float64."""
    indices = np.asarray(indices, dtype=np.int64)
    dx = np.zeros((n_src, dout.shape[1]), dtype=np.float64)
    r, f = np.nonzero(arg >= 0)
    np.add.at(dx, (indices[arg[r, f]], f), dout[r, f].astype(np.float64))
    return dx


def csc_of(g):
    """(indptr, indices) of a graph's CSC as numpy arrays."""
    return g.csc.indptr.cpu().numpy(), g.csc.indices.cpu().numpy()


def check_arg(indptr, arg):
    """Every arg entry is -1 or a position inside its row."""
    lo, hi = np.asarray(indptr[:-1])[:, None], np.asarray(indptr[1:])[:, None]
    assert np.all((arg == -1) | ((arg >= lo) & (arg < hi)))


# ------------------------------------------------------------------------------------------------ CPU stand-ins
def spmm_max_standin(d, x, relu=False, out=None, arg=None, workspace=None):
    o, a = max_forward(d.indptr.numpy(), d.indices.numpy(), x.detach().numpy(), relu)
    o, a = torch.from_numpy(o), torch.from_numpy(a)
    if out is not None:
        out.copy_(o)
        o = out
    if arg is not None:
        arg.copy_(a)
        a = arg
    return o, a


def spmm_max_bwd_standin(d_t, pos, dout, arg, out=None, partial=None):
    """The CSR-side definition itself, not `max_backward`: dx[u] = sum over u's out-edges j of dout[v_j] * (arg[v_j] == pos[j])."""
    rows = torch.repeat_interleave(torch.arange(d_t.n_rows), (d_t.indptr[1:] - d_t.indptr[:-1]).long())
    v = d_t.indices.long()
    hit = arg[v] == pos.reshape(-1, 1)
    dx = torch.zeros((d_t.n_rows, dout.shape[1]), dtype=dout.dtype).index_add(0, rows, torch.where(hit, dout[v], torch.zeros((), dtype=dout.dtype)))
    if out is not None:
        out.copy_(dx)
        return out
    return dx


def install(monkeypatch):
    from bot_amd import _C
    monkeypatch.setattr(_C, "spmm_max", spmm_max_standin)
    monkeypatch.setattr(_C, "spmm_max_bwd", spmm_max_bwd_standin)


# ------------------------------------------------------------------------------------------------ the aggregators, float64 torch
def relu_max(src, dst, n_dst, z, arg=None, pos_src=None):
    """max over the in-edges of relu(z[u]), 0 for a destination without in-edges: differentiable, float64.  With `arg` ([n_dst, F] CSC
    positions, -1 = none) and `pos_src` (the source of every CSC position) it is evaluated AT that choice: z[pos_src[arg]] where
    arg >= 0, else 0 - the function whose autograd gradient is the kernel's routing."""
    if arg is None:
        idx = dst.reshape(-1, 1).expand(-1, z.shape[1])
        return torch.zeros((n_dst, z.shape[1]), dtype=z.dtype).scatter_reduce(0, idx, torch.relu(z)[src], "amax", include_self=True)
    a = torch.as_tensor(arg).long()
    u = torch.as_tensor(pos_src).long()[a.clamp(min=0)]
    return torch.where(a >= 0, z.gather(0, u), torch.zeros((), dtype=z.dtype))


def _lin(x, p, name):
    y = x @ p[name + ".weight"].t()
    b = p.get(name + ".bias")
    return y if b is None else y + b


def sage_conv(kind, src, dst, n_src, n_dst, h_src, h_dst, p, out_feats, ew=None, arg=None, pos_src=None, pooled=None):
    """`SAGEConv(kind)` in float64.  src / dst: int64 edge lists; h_src [n_src, fin], h_dst [n_dst, fin_dst]; p: the
    layer's state_dict as float64 tensors; ew: per-edge weight in the order of src / dst.  `arg` / `pos_src`: evaluate the pool
    aggregator at the kernel's argmax (`relu_max`).  `pooled`: a list that receives fc_pool(h_src) (the operand of the max)."""
    before = h_src.shape[1] > out_feats
    deg = torch.bincount(dst, minlength=n_dst).to(F64)
    w = None if ew is None else ew.reshape(-1, 1)

    def total(x):
        msg = x[src] if w is None else x[src] * w
        return torch.zeros((n_dst, x.shape[1]), dtype=F64).index_add(0, dst, msg)
    if kind == "mean":
        inv = torch.where(deg > 0, 1.0 / deg.clamp(min=1), torch.zeros_like(deg))[:, None]
        h_neigh = total(_lin(h_src, p, "fc_neigh")) * inv if before else _lin(total(h_src) * inv, p, "fc_neigh")
        return _lin(h_dst, p, "fc_self") + h_neigh
    if kind == "gcn":
        inv = (1.0 / (deg + 1.0))[:, None]
        if before:
            return (total(_lin(h_src, p, "fc_neigh")) + _lin(h_dst, p, "fc_neigh")) * inv
        return _lin((total(h_src) + h_dst) * inv, p, "fc_neigh")
    assert kind == "pool" and ew is None
    z = _lin(h_src, p, "fc_pool")
    if pooled is not None:
        pooled.append(z)
    return _lin(h_dst, p, "fc_self") + _lin(relu_max(src, dst, n_dst, z, arg, pos_src), p, "fc_neigh")


def params64(module):
    """A module's parameters as float64 leaves, keyed like its state_dict."""
    return {k: v.detach().cpu().double().clone().requires_grad_() for k, v in module.named_parameters()}


def layer_params(p, i):
    pre = f"convs.{i}."
    return {k[len(pre):]: v for k, v in p.items() if k.startswith(pre)}


def sage_stack(model, layers, feat, p, args=None):
    """`GraphSAGE` in eval mode (no dropout, BatchNorm by its running statistics) in float64.  layers: per layer (src, dst, n_src,
    n_dst, ew or None, pos_src); args: per layer the kernel's arg for the pool aggregator, or None."""
    h = feat
    n_layers = len(model.convs)
    for i, (src, dst, n_src, n_dst, ew, pos_src) in enumerate(layers):
        conv = model.convs[i]
        h = sage_conv(conv._aggre_type, src, dst, n_src, n_dst, h, h[:n_dst], layer_params(p, i), conv._out_feats, ew,
                      None if args is None else args[i], pos_src)
        if i < n_layers - 1:
            if len(model.norms):
                bn = model.norms[i]
                h = (h - bn.running_mean.cpu().double()) * torch.rsqrt(bn.running_var.cpu().double() + bn.eps) * p[f"norms.{i}.weight"] + p[f"norms.{i}.bias"]
            h = torch.relu(h)
    return h


# ------------------------------------------------------------------------------------------------ shared graphs and checks
def small_graph(n_dst, n_src, seed, chunk=None):
    """A graph for the kernel tests: every fifth destination isolated, one destination with 40 in-edges, the others 1 .. 11, sources
    drawn with replacement (parallel edges happen, and five edges are doubled on purpose); n_src > n_dst makes it a block.  `chunk`: the
    row plans' chunk (4 turns every row above four edges into a long row, so the chunk and combine kernels run at small sizes)."""
    import bot_amd
    rng = np.random.default_rng(seed)
    deg = rng.integers(1, 12, n_dst)
    deg[np.arange(n_dst) % 5 == 2] = 0
    if n_dst > 3:
        deg[3] = 40
    if n_dst == 1:
        deg[0] = 7
    dst = np.repeat(np.arange(n_dst), deg)
    src = rng.integers(0, n_src, dst.size)
    src, dst = np.concatenate([src, src[:5]]), np.concatenate([dst, dst[:5]])
    order = rng.permutation(dst.size)                 # edge ids in no particular order
    return bot_amd.Graph(torch.from_numpy(src[order]), torch.from_numpy(dst[order]), n_src, num_dst_nodes=n_dst, chunk=chunk)


def sweep_edges(seed=7):
    """(src, dst, n) of the gather kernels' edge-case graph: 80 nodes; rows of 0, 1, 3, 4, 5, 63, 64, 65 and 20 in-edges (the batch of
    four and its tail; one id short of, exactly and one id past a group of 64 ids where the row plan's chunk leaves the rows whole), the
    others 0 .. 12; sources drawn with replacement and the last seven edges doubled on purpose; edge ids in no particular order."""
    rng = np.random.default_rng(seed)
    n = 80
    deg = rng.integers(0, 13, n)
    deg[:9] = [0, 1, 3, 4, 5, 63, 64, 65, 20]
    dst = np.repeat(np.arange(n), deg)
    src = rng.integers(0, n, dst.size)
    src, dst = np.concatenate([src, src[-7:]]), np.concatenate([dst, dst[-7:]])
    order = rng.permutation(dst.size)
    return torch.from_numpy(src[order]), torch.from_numpy(dst[order]), n


def tie_values(n, F, seed):
    """float32 [n, F] drawn from the integers -2 .. 2 with half of the zeros negative: most (row, column) pairs of a max tie."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-2, 3, (n, F)).astype(np.float32)
    x[(x == 0) & (rng.random((n, F)) < 0.5)] = -0.0
    return x


class Spy:
    """Counts `_C.spmm` calls and records `_C.spmm_max` calls (relu flag, returned arg) while active."""

    def __init__(self, monkeypatch):
        from bot_amd import _C
        self.spmm, self.max = 0, []
        real_spmm, real_max = _C.spmm, _C.spmm_max

        def spmm(*a, **k):
            self.spmm += 1
            return real_spmm(*a, **k)

        def spmm_max(d, x, relu=False, **k):
            out, arg = real_max(d, x, relu, **k)
            self.max.append((bool(relu), arg))
            return out, arg
        monkeypatch.setattr(_C, "spmm", spmm)
        monkeypatch.setattr(_C, "spmm_max", spmm_max)


def edge_lists(g):
    """(src, dst, n_src, n_dst, source of every CSC position) of a graph, on the CPU."""
    src, dst = (t.cpu().long() for t in g.edges())
    return src, dst, g.number_of_src_nodes(), g.number_of_dst_nodes(), g.csc.indices.cpu().long()


def check_conv(g, dev, kind, fin, fout, weighted, monkeypatch, seed=0):
    """One `SAGEConv(kind)` forward + backward on `g` against `sage_conv` under the suite's own criteria (tests/parity_cases.py): the
    output, and the gradients of the input, every weight and bias and (weighted) the edge weight.  pool: the restatement is evaluated at
    the kernel's arg, and that arg must be a near-maximiser in float64 (the forward criterion applied to both operands).  Also the
    launch contract: mean and gcn make ONE sparse launch per forward, pool calls the max kernel once with relu on."""
    from bot_amd import nn as bnn
    from tests.parity_cases import FWD_ATOL, fwd_close, grad_close
    src, dst, n_src, n_dst, pos_src = edge_lists(g)
    gen = torch.Generator().manual_seed(seed)
    torch.manual_seed(seed)
    conv = bnn.SAGEConv(fin, fout, kind)
    with torch.no_grad():
        for name, prm in conv.named_parameters():
            if name.endswith("bias"):
                prm.copy_(torch.randn(prm.shape, generator=gen))
    conv = conv.to(dev)
    feat = torch.randn(n_src, fin, generator=gen).to(dev).requires_grad_()
    dout = torch.randn(n_dst, fout, generator=gen)
    ew = (0.25 + 1.5 * torch.rand(src.numel(), generator=gen)) if weighted else None
    ewl = None if ew is None else ew.clone().to(dev).requires_grad_()
    spy = Spy(monkeypatch)
    out = conv(g, feat) if ewl is None else conv(g, feat, edge_weight=ewl)
    if kind == "pool":
        assert spy.spmm == 0 and [r for r, _ in spy.max] == [True]
    else:
        assert spy.spmm == 1 and spy.max == []
    out.backward(dout.to(dev))
    p = params64(conv)
    f64 = feat.detach().cpu().double().requires_grad_()
    e64 = None if ew is None else ew.double().requires_grad_()
    arg = None if kind != "pool" else spy.max[0][1].cpu()[:, :fin]
    pooled = []
    ref = sage_conv(kind, src, dst, n_src, n_dst, f64, f64[:n_dst], p, fout, e64, arg, pos_src, pooled)
    ref.backward(dout.double())
    assert out.shape == (n_dst, fout)
    fwd_close(out, ref.detach().numpy())
    grad_close(feat.grad, f64.grad.numpy())
    for name, prm in conv.named_parameters():
        grad_close(prm.grad, p[name].grad.numpy())
    if weighted:
        grad_close(ewl.grad, e64.grad.numpy())
    if kind == "pool":
        z64 = pooled[0].detach()
        check_arg(g.csc.indptr.cpu().numpy(), arg.numpy())
        assert bool((relu_max(src, dst, n_dst, z64, arg, pos_src) >= relu_max(src, dst, n_dst, z64) - 2 * FWD_ATOL).all())
    return conv


def check_stack(model, graphs, feat, dev, monkeypatch, edge_weight=None):
    """`GraphSAGE` in eval mode on a Graph (graphs: the graph) or a block list against `sage_stack`: output, input gradient and every
    parameter's gradient; pool layers are evaluated at the kernel's arg."""
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
    spy = Spy(monkeypatch)
    out = model(graphs, x) if edge_weight is None else model(graphs, x, edge_weight=edge_weight)
    gen = torch.Generator().manual_seed(12)
    dout = torch.randn(out.shape, generator=gen)
    out.backward(dout.to(dev))
    p = params64(model)
    f64 = feat.detach().cpu().double().requires_grad_()
    layers, args = [], []
    pool = model.convs[0]._aggre_type == "pool"
    for i, g in enumerate(per_layer):
        src, dst, n_src, n_dst, pos_src = edge_lists(g)
        w = None if edge_weight is None else (edge_weight if blocks is None else edge_weight[i]).detach().cpu().double().reshape(-1)
        layers.append((src, dst, n_src, n_dst, w, pos_src))
        args.append(spy.max[i][1].cpu()[:, :model.convs[i]._in_src_feats] if pool else None)
    ref = sage_stack(model, layers, f64, p, args if pool else None)
    ref.backward(dout.double())
    fwd_close(out, ref.detach().numpy())
    grad_close(x.grad, f64.grad.numpy())
    for name, prm in model.named_parameters():
        grad_close(prm.grad, p[name].grad.numpy())
