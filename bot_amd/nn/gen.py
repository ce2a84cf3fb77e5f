"""DeeperGCN (Li, Xiong, Thabet, Ghanem, "DeeperGCN: All You Need to Train Deeper GCNs", arXiv:2006.07739): `GENConv` with the
softmax aggregator, in the shape of DGL's `dgl.nn.GENConv` where DESIGN §1 states it, and the `DeeperGCN` "res+" stack in `nn.GCN`'s shape.

The aggregation is `ops.copy_u_softmax` (csrc/spmm_softmax.hip): one online-softmax sweep per column with the message's
`relu(.) + eps` folded in front of it, so neither the [n_src, F] message pass nor anything of size [E, F] exists.  beta may be learned:
the kernels read it from device memory and its gradient is a dense reduction over saved row statistics.  With `edge_dim=K` the layer
owns the edge encoder and the aggregation is `ops.u_add_e_softmax` (csrc/spmm_softmax_edge.hip), which projects an edge's K raw features
inside the sweep.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..graph import take_rows
from . import _block_list, _epilogue, _sampled, _src_rows
from .sage import _position_order

__all__ = ["GENConv", "DeeperGCN"]

MLP_EXPANSION = 2     # hidden width of the layer's MLP over its input width (DGL's and PyG's default)


class GENConv(nn.Module):
    """Generalised aggregation layer (DGL's `GENConv`):

        m_u    = relu(h_u) + eps                    (with edge_feats: relu(h_u + ef_e) + eps per edge e = u -> v)
        h_agg  = sum over the in-edges of softmax_u(beta m_u) m_u, per destination and column; 0 without in-edges
        h_agg  = normalize(h_agg, p=2) * ||h_dst||_2 * msg_scale                                      (msg_norm)
        rst    = mlp(h_dst + h_agg)

    The MLP is `mlp_layers` Linear layers, in_feats -> 2 in_feats -> ... -> out_feats, with `norm -> ReLU` between them ("batch",
    "layer" or "none").  `beta`: a float, or with `learn_beta` a one-element parameter.  `msg_scale` exists with `msg_norm` and is
    trained with `learn_msg_scale`.  `graph`: a whole Graph, a Subgraph or a sampled Block (destinations = the first n_dst source
    rows); `feat`: a tensor or a (feat_src, feat_dst) pair.  `edge_feats` without `edge_dim`: float32 [E, in_feats] in edge-id order,
    already encoded; the layer then runs the tensor form whatever `ops.softmax_agg_default_impl` says (the kernel form with a per-edge
    operand is the one below: DESIGN §8).  `edge_dim=K`: the layer owns `lin_edge = nn.Linear(K, in_feats)` (PyG's name), `edge_feats`
    is the RAW float32 [E, K] in edge-id order and must be given, and ef_e = lin_edge(edge_feats[e]) is formed inside the sweep of
    `ops.u_add_e_softmax`: nothing of size [E, in_feats] exists.  aggregator "power" is not built (NotImplementedError).  A partition with
    a halo plan raises ValueError."""

    def __init__(self, in_feats, out_feats, aggregator="softmax", beta=1.0, learn_beta=False, msg_norm=False, learn_msg_scale=False,
                 mlp_layers=1, eps=1e-7, norm="batch", edge_dim=None):
        super().__init__()
        if aggregator == "power":
            raise NotImplementedError("GENConv: the power-mean aggregator is not built (DESIGN §8); use softmax")
        if aggregator != "softmax":
            raise ValueError(f'GENConv: aggregator must be "softmax" (or "power", not built), got {aggregator!r}')
        if norm not in ("batch", "layer", "none"):
            raise ValueError(f'norm must be "batch", "layer" or "none", got {norm!r}')
        if mlp_layers < 1:
            raise ValueError(f"mlp_layers must be at least 1, got {mlp_layers}")
        if edge_dim is not None and int(edge_dim) < 1:
            raise ValueError(f"edge_dim must be at least 1, got {edge_dim}")
        self._in_feats, self._out_feats, self.aggregator, self.eps = in_feats, out_feats, aggregator, float(eps)
        self._edge_dim = None if edge_dim is None else int(edge_dim)
        if self._edge_dim is not None:
            self.lin_edge = nn.Linear(self._edge_dim, in_feats)
        if learn_beta:
            self.beta = nn.Parameter(torch.tensor([float(beta)]))
        else:
            self.beta = float(beta)
        if msg_norm:
            self.msg_scale = nn.Parameter(torch.tensor([1.0]), requires_grad=bool(learn_msg_scale))
        else:
            self.msg_scale = None
        widths = [in_feats] + [in_feats * MLP_EXPANSION] * (mlp_layers - 1) + [out_feats]
        self.mlp, self.mlp_norms = nn.ModuleList(), nn.ModuleList()
        for i in range(mlp_layers):
            self.mlp.append(nn.Linear(widths[i], widths[i + 1]))
            if i < mlp_layers - 1:
                self.mlp_norms.append({"batch": nn.BatchNorm1d, "layer": nn.LayerNorm, "none": lambda w: nn.Identity()}[norm](widths[i + 1]))
        self._no_drop = nn.Dropout(0.0)

    def forward(self, graph, feat, edge_feats=None):
        if graph.halo is not None:
            raise ValueError("GENConv on a partitioned graph (a halo plan) is not supported: it takes whole graphs, Subgraphs and "
                             "sampled blocks")
        n_dst = graph.number_of_dst_nodes()
        if isinstance(feat, tuple):
            h_src, h_dst = _src_rows(graph, feat[0]), feat[1]
            if h_dst.shape[0] != n_dst:
                raise ValueError(f"feat_dst holds {h_dst.shape[0]} rows, the graph has {n_dst} destination nodes")
        else:
            h_src = _src_rows(graph, feat)
            h_dst = h_src[:n_dst] if _sampled(graph) else h_src      # a block's destinations are its first n_dst sources
        if h_src.dim() != 2 or h_src.shape[1] != self._in_feats or h_dst.shape[1:] != h_src.shape[1:]:
            raise ValueError(f"GENConv({self._in_feats}, {self._out_feats}) takes [n, {self._in_feats}] features, got "
                             f"{tuple(h_src.shape)} and {tuple(h_dst.shape)}")
        if self._edge_dim is not None:
            E = graph.number_of_edges()
            if edge_feats is None:
                raise ValueError(f"GENConv(edge_dim={self._edge_dim}) needs edge_feats [{E}, {self._edge_dim}]")
            if edge_feats.dim() != 2 or tuple(edge_feats.shape) != (E, self._edge_dim):
                raise ValueError(f"edge_feats must be [{E}, {self._edge_dim}] (one row of raw features per edge, edge-id order), got "
                                 f"{tuple(edge_feats.shape)}")
            h_agg = ops.u_add_e_softmax(graph, h_src, edge_feats, self.lin_edge.weight, self.lin_edge.bias, self.beta, relu=True, eps=self.eps)
        elif edge_feats is None:
            h_agg = ops.copy_u_softmax(graph, h_src, self.beta, relu=True, eps=self.eps)
        else:
            E = graph.number_of_edges()
            if edge_feats.shape != (E, self._in_feats):
                raise ValueError(f"edge_feats must be [{E}, {self._in_feats}] (one row per edge, edge-id order), got {tuple(edge_feats.shape)}")
            msg = torch.relu(take_rows(h_src, graph.csc.indices) + _position_order(graph, edge_feats)) + self.eps
            beta = self.beta.reshape(()) if isinstance(self.beta, torch.Tensor) else self.beta
            h_agg = ops.softmax_agg_positions(graph, msg, beta)
        if self.msg_scale is not None:
            h_agg = F.normalize(h_agg, p=2, dim=-1) * h_dst.norm(p=2, dim=-1, keepdim=True) * self.msg_scale
        h = h_dst + h_agg
        for i, fc in enumerate(self.mlp):
            h = ops.linear(h, fc.weight, fc.bias)
            if i < len(self.mlp) - 1:
                h = _epilogue(h, self.mlp_norms[i], F.relu, self._no_drop, self.training)
        return h

    def extra_repr(self):
        edge = "" if self._edge_dim is None else f", edge_dim={self._edge_dim}"
        return f"in={self._in_feats}, out={self._out_feats}, aggregator={self.aggregator}, eps={self.eps}{edge}"


def layer_edge_feats(who, edge_dim, n_layers, graph, blocks, edge_feats):
    """Per layer the raw edge features of its graph for a stack `who` with `edge_dim` (`DeeperGCN`, `EdgeUniMP`), or None per layer
    without `edge_dim`.  A Graph or Subgraph (`blocks` None): `edge_feats` a tensor, an `edata` key or None for edata["feat"]; a block
    list: a list of one tensor per block, or None for each block's rows of the parent's column."""
    if edge_dim is None:
        if edge_feats is not None:
            raise ValueError(f"{who} takes edge_feats only with edge_dim")
        return [None] * n_layers
    if blocks is None:
        if edge_feats is None or isinstance(edge_feats, str):
            key = "feat" if edge_feats is None else edge_feats
            if key not in graph.edata:
                raise ValueError(f"{who}(edge_dim={edge_dim}) needs edge_feats: the graph has no edata[{key!r}]")
            edge_feats = graph.edata[key]
        return [edge_feats] * n_layers
    if edge_feats is None:
        return [b.edata["feat"] for b in blocks]                 # each block's rows of the parent's column
    if not isinstance(edge_feats, (list, tuple)) or len(edge_feats) != n_layers:
        raise ValueError(f"a block list takes edge_feats as a list of {n_layers} tensors (one per block)")
    return list(edge_feats)


class DeeperGCN(nn.Module):
    """The "res+" stack of the DeeperGCN paper over `GENConv` layers of one width:

        h = node_encoder(feat);   h = conv_0(g, h);   h = conv_i(g, dropout(relu(norm_i(h)))) + h   for i >= 1;
        out = output(dropout(relu(norm(h))))

    with BatchNorm1d norms (BatchNorm + ReLU + dropout run as the fused epilogue).  With `msg_norm` every layer's `msg_scale` is trained
    (`learn_msg_scale=True`, the paper's MsgNorm; the stack has no separate switch for it).  `forward` has `GCN.forward`'s contract: a Graph with
    its node features in original order, or a list of n_layers sampled blocks, where the residual takes the destination prefix of its
    input; so the stack runs under train.train_step, minibatch.train_epoch, minibatch.subgraph_step and train_epoch_subgraphs
    unchanged.  With `edge_dim=K` every layer is a `GENConv(edge_dim=K)` with its own `lin_edge`, and `forward` hands each layer the raw
    edge features of its graph (by default the column edata["feat"])."""

    def __init__(self, in_feats, n_classes, n_hidden, n_layers, dropout=0.0, beta=1.0, learn_beta=False, msg_norm=False, mlp_layers=1,
                 input_drop=0.0, edge_dim=None):
        super().__init__()
        if n_layers < 1:
            raise ValueError(f"n_layers must be at least 1, got {n_layers}")
        self.n_layers, self.n_hidden, self.n_classes, self.edge_dim = n_layers, n_hidden, n_classes, edge_dim
        self.node_encoder = nn.Linear(in_feats, n_hidden)
        self.convs = nn.ModuleList(GENConv(n_hidden, n_hidden, beta=beta, learn_beta=learn_beta, msg_norm=msg_norm,
                                           learn_msg_scale=msg_norm, mlp_layers=mlp_layers, edge_dim=edge_dim) for _ in range(n_layers))
        self.norms = nn.ModuleList(nn.BatchNorm1d(n_hidden) for _ in range(n_layers))     # norms[i - 1] in front of conv_i; the last in front of the output
        self.output = nn.Linear(n_hidden, n_classes)
        self.input_drop, self.dropout = nn.Dropout(input_drop), nn.Dropout(dropout)

    def _edge_feats(self, graph, blocks, edge_feats):
        return layer_edge_feats(type(self).__name__, self.edge_dim, self.n_layers, graph, blocks, edge_feats)

    def forward(self, graph, feat=None, edge_feats=None):
        """`graph`: a Graph (`feat` in original node order), or a list of n_layers sampled blocks: layer i runs on blocks[i], `feat`
        defaults to blocks[0].srcdata["feat"].  `edge_feats` (with `edge_dim`; raw [E, edge_dim] in edge-id order): for a Graph or
        Subgraph a tensor, an `edata` key or None for edata["feat"]; for a block list a list of one tensor per block, or None for each
        block's rows of the parent's edata["feat"]."""
        blocks = _block_list(graph, feat, self.n_layers)
        efs = self._edge_feats(graph, blocks, edge_feats)
        h = graph.to_internal(feat) if blocks is None else (blocks[0].srcdata["feat"] if feat is None else feat)
        h = self.input_drop(h)
        h = ops.linear(h, self.node_encoder.weight, self.node_encoder.bias)
        for i in range(self.n_layers):
            g = graph if blocks is None else blocks[i]
            if i == 0:
                h = self.convs[0](g, h, efs[0])
                continue
            t = _epilogue(h, self.norms[i - 1], F.relu, self.dropout, self.training)
            h = self.convs[i](g, t, efs[i]) + (h if blocks is None else h[:g.number_of_dst_nodes()])
        h = _epilogue(h, self.norms[self.n_layers - 1], F.relu, self.dropout, self.training)
        h = ops.linear(h, self.output.weight, self.output.bias)
        return h if blocks is not None else graph.to_original(h)
