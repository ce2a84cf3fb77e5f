"""Checks of the GCN / GAT layers and stacks on sampled blocks (bot_amd.nn on bot_amd.sampling blocks, the fused nodes of
bot_amd/nn/fused.py included), shared by tests/test_block_stacks_host.py (emulated backend, blocks built by `host_blocks`) and
tests/test_block_stacks_gpu.py (MI355X, blocks from the on-device sampler).

The oracle (oracle/ref_models.py) runs in float64 on the block seen as an n_src-node graph whose rows from n_dst on have no in-edges;
its result is sliced to the n_dst destination rows (the reference's block branch, models.py:350, :493-495)."""
import torch
import torch.nn.functional as F

import bot_amd
from bot_amd import nn as bnn
from bot_amd.sampling import Block
from oracle import ref_models as RM
from oracle import ref_ops as R


def close(a, b, tol, what=""):
    """max |a - b| <= tol x max |b| (the block tests' measure)."""
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    scale = max(float(b.abs().max()), 1e-30) if b.numel() else 1.0
    err = float((a - b).abs().max()) / scale if b.numel() else 0.0
    assert a.shape == b.shape and err <= tol, (what, tuple(a.shape), tuple(b.shape), err)


def parent_graph(device, n=600, e_raw=4000, seed=5, fin=8, n_classes=5):
    """A preprocessed power-law graph (self-loops: no destination is without in-edges) with `feat` [n, fin] and the one-hot
    `train_labels_onehot` of the first half of the nodes."""
    from bot_amd import synth
    rs, rd = synth.powerlaw_edges(n, e_raw, seed)
    s, d = R.preprocess_edges(rs, rd, n)
    g = bot_amd.Graph(s, d, n).to(device)
    gen = torch.Generator().manual_seed(seed + 1)
    g.ndata["feat"] = torch.randn(n, fin, generator=gen).to(device)
    labels = torch.randint(0, n_classes, (n,), generator=gen)
    onehot = torch.zeros(n, n_classes)
    onehot[torch.arange(n // 2), labels[:n // 2]] = 1.0
    g.ndata["train_labels_onehot"] = onehot.to(device)
    return g


def host_blocks(g, seeds, fanouts, seed=0):
    """Blocks input layer first, built with torch ops from the parent's CSC (the sampler's output contract, any device): in-edges of a
    destination uniformly without replacement (fanout -1: all), destinations first, new sources in ascending parent id."""
    gen = torch.Generator().manual_seed(seed)
    csc = g.csc
    indptr, indices, eid = csc.indptr.long().cpu(), csc.indices.long().cpu(), csc.eid.long().cpu()
    seeds = torch.as_tensor(seeds).long().cpu()
    blocks = []
    for k in reversed(list(fanouts)):
        pos, offsets = [], [0]
        for v in seeds.tolist():
            lo, hi = int(indptr[v]), int(indptr[v + 1])
            take = torch.arange(lo, hi)
            if 0 <= k < hi - lo:
                take = lo + torch.sort(torch.randperm(hi - lo, generator=gen)[:k]).values
            pos.append(take)
            offsets.append(offsets[-1] + take.numel())
        pos = torch.cat(pos)
        src_parent = indices[pos]
        new = torch.unique(src_parent[~torch.isin(src_parent, seeds)])
        src_nid = torch.cat([seeds, new])
        local = torch.full((g.number_of_nodes(),), -1, dtype=torch.int64)
        local[src_nid] = torch.arange(src_nid.numel())
        dev = g.device
        b = Block(g, src_nid.to(dev, torch.int32), torch.tensor(offsets, dtype=torch.int32, device=dev),
                  local[src_parent].to(dev, torch.int32).contiguous(), eid[pos].to(dev, torch.int32))
        blocks.insert(0, b)
        seeds = src_nid
    return blocks


def coo(b):
    s, d = (t.cpu() for t in b.edges())
    return RM.CooGraph(s, d, b.number_of_src_nodes())


def f64(module):
    """float64 CPU copies of the state_dict; the parameters' copies are leaves that take gradients."""
    params = {k for k, _ in module.named_parameters()}
    return {k: (v.detach().cpu().double().requires_grad_(k in params) if v.is_floating_point() else v.cpu())
            for k, v in module.state_dict().items()}


def _grads_match(module, sd, tol, skip=()):
    for k, p in module.named_parameters():
        if k in skip:
            continue
        close(p.grad, sd[k].grad, tol, k)


# ------------------------------------------------------------------------------------------------ layers
def check_graphconv_on_block(b, device, norm, fin, fout, train):
    nd, ns = b.number_of_dst_nodes(), b.number_of_src_nodes()
    torch.manual_seed(11)
    conv = bnn.GraphConv(fin, fout, norm=norm).to(device).train(train)
    with torch.no_grad():
        conv.bias.normal_()
    x = torch.randn(ns, fin, generator=torch.Generator().manual_seed(4)).to(device)
    gout = torch.randn(nd, fout, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    sd = f64(conv)
    xr = x.cpu().double().requires_grad_()
    ref = RM.graphconv_forward(coo(b), xr, sd["weight"], sd["bias"], norm, allow_zero_in_degree=True)[:nd]
    (ref * gout).sum().backward()
    xg = x.clone().requires_grad_()
    out = conv(b, xg)
    assert out.shape == (nd, fout)
    close(out, ref, 1e-4, "out")
    (out * gout.to(device, torch.float32)).sum().backward()
    close(xg.grad, xr.grad, 2e-4, "dx")
    _grads_match(conv, sd, 2e-4)


def check_gatconv_on_block(b, device, sym, attn_r, res, train, keep=False, H=3, D=6, fin=10):
    nd, ns, E = b.number_of_dst_nodes(), b.number_of_src_nodes(), b.number_of_edges()
    torch.manual_seed(12)
    conv = bnn.GATConv(fin, D, num_heads=H, edge_drop=0.3 if keep else 0.0, use_symmetric_norm=sym, non_interactive_attn=attn_r,
                       linear=res).to(device).train(train)
    x = torch.randn(ns, fin, generator=torch.Generator().manual_seed(4)).to(device)
    gout = torch.randn(nd, H, D, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
    km = kept = None
    if keep:
        km = (torch.rand(E, generator=torch.Generator().manual_seed(8)) >= 0.3).to(torch.uint8)
        kept = torch.nonzero(km).squeeze(1)
        km = km.to(device)
    sd = f64(conv)
    xr = x.cpu().double().requires_grad_()
    ref = RM.gatconv_forward(coo(b), xr, sd["fc.weight"], sd["attn_l"], sd["attn_r"] if attn_r else None,
                             sd["res_fc.weight"] if res else None, num_heads=H, out_feats=D, use_symmetric_norm=sym,
                             keep_eids=kept, allow_zero_in_degree=True)[:nd]
    (ref * gout).sum().backward()
    xg = x.clone().requires_grad_()
    out = conv(b, xg, keep=km)
    assert out.shape == (nd, H, D)
    close(out, ref, 1e-4, "out")
    (out * gout.to(device, torch.float32)).sum().backward()
    close(xg.grad, xr.grad, 2e-4, "dx")
    _grads_match(conv, sd, 2e-4)


def _gat_pair_reference(b, xs, xd, Ws, Wd, attn_l, attn_r, Wres, H, D):
    """models.py:481-488 + :517-560 in float64 on the block: el from fc_src(feat_src), er from fc_dst(feat_dst), res_fc(feat_dst)."""
    g = coo(b)
    nd = b.number_of_dst_nodes()
    ft = F.linear(xs, Ws).view(-1, H, D)
    fd = F.linear(xd, Wd).view(-1, H, D)
    el = (ft * attn_l).sum(-1, keepdim=True)
    er = (fd * attn_r).sum(-1, keepdim=True)
    e = F.leaky_relu(R.u_add_v(g.src, g.dst, el, torch.cat([er, er.new_zeros((g.num_nodes - nd,) + er.shape[1:])])), 0.2)
    a = R.edge_softmax(g.dst, g.num_nodes, e)
    rst = R.u_mul_e_sum(g.src, g.dst, g.num_nodes, ft, a)[:nd]
    return rst + F.linear(xd, Wres).view(nd, H, D)


def check_tuple_features(g, b, device):
    """GraphConv and GATConv given (feat_src, feat_dst): on a block and on a whole graph."""
    nd, ns = b.number_of_dst_nodes(), b.number_of_src_nodes()
    gen = torch.Generator().manual_seed(21)
    x = torch.randn(ns, 10, generator=gen).to(device)
    torch.manual_seed(13)
    gc = bnn.GraphConv(10, 7).to(device)
    assert torch.equal(gc(b, (x, x[:nd])), gc(b, x))
    n = g.number_of_nodes()
    xg = torch.randn(n, 10, generator=gen).to(device)
    assert torch.equal(gc(g, (xg, xg)), gc(g, xg))
    # a GATConv built with one input size takes the pair through its `fc` (and keeps its state_dict keys)
    torch.manual_seed(14)
    conv = bnn.GATConv(10, 6, num_heads=2, non_interactive_attn=True).to(device)
    keys = set(conv.state_dict())
    close(conv(b, (x, x[:nd])), conv(b, x), 1e-6, "pair = block")
    close(conv(g, (xg, xg)), conv(g, xg), 1e-6, "pair = graph")
    assert set(conv.state_dict()) == keys and not hasattr(conv, "fc_src")
    # a GATConv built with (in_src, in_dst): fc_src / fc_dst, against the float64 restatement, forward and gradients
    torch.manual_seed(15)
    conv = bnn.GATConv((10, 4), 6, num_heads=2, non_interactive_attn=True).to(device)
    for graph, xs in ((b, x), (g, xg)):
        xd = torch.randn(graph.number_of_dst_nodes(), 4, generator=gen).to(device)
        sd = f64(conv)
        xsr, xdr = xs.cpu().double().requires_grad_(), xd.cpu().double().requires_grad_()
        src_b = graph if graph is b else _whole_as_block(graph)
        ref = _gat_pair_reference(src_b, xsr, xdr, sd["fc_src.weight"], sd["fc_dst.weight"], sd["attn_l"], sd["attn_r"],
                                  sd["res_fc.weight"], 2, 6)
        gout = torch.randn(ref.shape, generator=gen, dtype=torch.float64)
        (ref * gout).sum().backward()
        conv.zero_grad()
        xsg, xdg = xs.clone().requires_grad_(), xd.clone().requires_grad_()
        out = conv(graph, (xsg, xdg))
        close(out, ref, 1e-4, "pair out")
        (out * gout.to(device, torch.float32)).sum().backward()
        close(xsg.grad, xsr.grad, 2e-4, "d feat_src")
        close(xdg.grad, xdr.grad, 2e-4, "d feat_dst")
        _grads_match(conv, sd, 2e-4)


class _whole_as_block:
    """A whole graph under the two methods `_gat_pair_reference` asks of a block."""

    def __init__(self, g):
        self._g = g

    def edges(self):
        return self._g.edges()

    def number_of_src_nodes(self):
        return self._g.number_of_nodes()

    def number_of_dst_nodes(self):
        return self._g.number_of_nodes()


# ------------------------------------------------------------------------------------------------ stacks
N_CLASSES = 5


def gat_stack(device, fin, sym, hidden=16):
    """Config-2-shaped, small: 3 layers x 3 heads, BatchNorm, linear (res_fc), label columns in the input (fin = features + classes:
    layer 0 is narrower than one head -> the aggregate-first node)."""
    torch.manual_seed(7)
    m = bnn.GAT(dim_node=fin, dim_edge=0, dim_output=N_CLASSES, n_hidden=hidden, n_layers=3, n_heads=3, activation=F.relu, norm="batch",
                dropout=0.0, input_drop=0.0, attn_drop=0.0, edge_drop=0.0, use_symmetric_norm=sym, linear=True)
    return m.to(device)


def gcn_stack(device, fin, residual, use_linear=False):
    torch.manual_seed(9)
    m = bnn.GCN(in_feats=fin, n_classes=N_CLASSES, n_hidden=12, n_layers=3, activation=F.relu, norm="batch", norm_adj="symm",
                dropout=0.0, residual=residual, use_linear=use_linear)
    return m.to(device)


def _bn(h, sd, i, train):
    if train:
        return F.batch_norm(h, None, None, sd[f"norms.{i}.weight"], sd[f"norms.{i}.bias"], training=True)
    return F.batch_norm(h, sd[f"norms.{i}.running_mean"], sd[f"norms.{i}.running_var"], sd[f"norms.{i}.weight"], sd[f"norms.{i}.bias"],
                        training=False)


def oracle_gat_on_blocks(blocks, feat, sd, sym, train, hidden=16):
    """GAT.forward (models.py:709-736) on a list of blocks, the oracle's layer per block."""
    h = feat
    n = len(blocks)
    for i, b in enumerate(blocks):
        nd = b.number_of_dst_nodes()
        last = i == n - 1
        h = RM.gatconv_forward(coo(b), h, sd[f"convs.{i}.fc.weight"], sd[f"convs.{i}.attn_l"], None, sd[f"convs.{i}.res_fc.weight"],
                               num_heads=1 if last else 3, out_feats=N_CLASSES if last else hidden, use_symmetric_norm=sym,
                               allow_zero_in_degree=True)[:nd]
        if not last:
            h = F.relu(_bn(h.flatten(1), sd, i, train))
    return h.mean(1) + sd["biases.0.bias"]


def oracle_gcn_on_blocks(blocks, feat, sd, residual, train, use_linear=False):
    """GCN.forward (models.py:616-641) on a list of blocks: the skip paths take the destination prefix."""
    h, h_last = feat, None
    n = len(blocks)
    for i, b in enumerate(blocks):
        nd = b.number_of_dst_nodes()
        conv = RM.graphconv_forward(coo(b), h, sd[f"convs.{i}.weight"], sd.get(f"convs.{i}.bias"), "both", allow_zero_in_degree=True)[:nd]
        if use_linear:
            conv = conv + F.linear(h[:nd], sd[f"linear.{i}.weight"])
        h = conv
        if i < n - 1:
            if residual and h_last is not None:
                h = h + h_last[:nd]
            h_last = h
            h = F.relu(_bn(h, sd, i, train))
    return h


def run_stack_against_oracle(model, blocks, oracle, train, tol_out=1e-4, tol_grad=2e-4):
    """Logits (and in train mode every parameter gradient) of `model(blocks)` against `oracle(feat64, sd64)`.  Returns the logits."""
    model.train(train)
    dev = blocks[0].device
    sd = f64(model)
    feat = blocks[0].srcdata["feat"]
    ref = oracle(feat.cpu().double(), sd)
    if not train:
        with torch.no_grad():
            out = model(blocks)
        close(out, ref, tol_out, "eval logits")
        return out
    model.zero_grad(set_to_none=True)
    out = model(blocks)
    close(out, ref, tol_out, "logits")
    gout = torch.randn(ref.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    (ref * gout).sum().backward()
    (out * gout.to(dev, torch.float32)).sum().backward()
    for k, p in model.named_parameters():
        if p.grad is None and sd[k].grad is None:
            continue
        scale = float(sd[k].grad.abs().max())
        if k.startswith("convs.") and k.endswith(".bias") and scale < 1e-6:
            # zero in exact arithmetic (a bias in front of a training-mode BatchNorm): fp32 cancellation noise only
            assert float(p.grad.abs().max()) < 1e-4, k
            continue
        close(p.grad, sd[k].grad, tol_grad, k)
    return out.detach()


def with_labels(g, fin):
    """The parent's input features with the label columns appended (the sampled --labels input: here every node's columns are the
    parent's `train_labels_onehot`), stored as ndata["feat"]."""
    g.ndata["feat"] = torch.cat([g.ndata["feat"][:, :fin], g.ndata["train_labels_onehot"]], 1)
    return g.ndata["feat"].shape[1]
