"""Dot-product attention layers: `DotGatConv` with the surface of DGL's `dgl.nn.DotGatConv`, `TransformerConv` with the surface and
parameter names of PyG's `torch_geometric.nn.TransformerConv` (the layer of UniMP: Shi et al., "Masked Label Prediction: Unified Message
Passing Model for Semi-Supervised Classification", IJCAI 2021, arXiv:2009.03509), and the `UniMP` stack in `nn.GATv2`'s shape.  `EdgeTransformerConv` is `TransformerConv(edge_dim=K)`: K raw edge features projected into the key and the value
(`ops.dot_attention_edge`, csrc/dot_attn.hip).

The layers are projections (`ops.linear`) around `ops.dot_attention`: on the GPU ONE fused sweep per forward that forms the logits,
the online softmax and the aggregation from one gather (csrc/dot_attn.hip), attention dropout included as a bit mask per edge.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops
from ..errors import DGLError
from . import _block_list, _epilogue, _pair, _sampled, _src_rows, has_zero_in_degree
from .gen import layer_edge_feats

__all__ = ["DotGatConv", "TransformerConv", "EdgeTransformerConv", "UniMP", "EdgeUniMP"]

_ZERO_IN_DEGREE = ("There are 0-in-degree nodes in the graph, output for those nodes will be invalid. "
                   "Adding self-loop on the input graph by calling `g = g.add_self_loop()` will resolve the issue. "
                   "Setting ``allow_zero_in_degree`` to be `True` when constructing this module will suppress the check.")


def _rows(layer, graph, feat, allow_zero_in_degree):
    """(h_src, h_dst) of a layer call on a Graph, a Subgraph or a sampled Block, `feat` a tensor or a (feat_src, feat_dst) pair; the
    checks of `GATv2Conv.forward`."""
    if graph.halo is not None:
        raise ValueError(f"{layer} on a partitioned graph (a halo plan) is not supported: it takes whole graphs, Subgraphs and sampled blocks")
    if not allow_zero_in_degree and has_zero_in_degree(graph):
        raise DGLError(_ZERO_IN_DEGREE)
    n_dst = graph.number_of_dst_nodes()
    if isinstance(feat, tuple):
        h_src, h_dst = _src_rows(graph, feat[0]), feat[1]
        if h_dst.shape[0] != n_dst:
            raise ValueError(f"feat_dst holds {h_dst.shape[0]} rows, the graph has {n_dst} destination nodes")
        return h_src, h_dst, False
    h_src = _src_rows(graph, feat)
    return h_src, (h_src[:n_dst] if _sampled(graph) else h_src), True      # a block's destinations are its first n_dst sources


class DotGatConv(nn.Module):
    """Dot-product attention layer (DGL's `DotGatConv`): one bias-free `fc`,

        k = v = fc(h_src),  q = fc(h_dst)                                        [n, H, D]
        a = softmax over the in-edges u -> v of (q[v] . k[u]) * out_feats ** -0.5;   rst[v] = sum_u a * v[u]        [n_dst, H, D]

    k and v are one tensor, so the sweep gathers one row per edge.  `graph`: a whole Graph, a Subgraph or a sampled Block; `feat`: a
    tensor or a (feat_src, feat_dst) pair.  `get_attention=True` runs the tensor form and also returns a [E, H, 1] in CSC position
    order.  A partition with a halo plan raises ValueError."""

    def __init__(self, in_feats, out_feats, num_heads, allow_zero_in_degree=False):
        super().__init__()
        self._in_src_feats, self._in_dst_feats = _pair(tuple(in_feats) if isinstance(in_feats, list) else in_feats)
        if self._in_src_feats != self._in_dst_feats:
            raise DGLError(f"DotGatConv has one fc for sources and destinations: equal widths, got {self._in_src_feats} and {self._in_dst_feats}")
        self._out_feats, self._num_heads, self._allow_zero_in_degree = out_feats, num_heads, allow_zero_in_degree
        self.fc = nn.Linear(self._in_src_feats, out_feats * num_heads, bias=False)

    def set_allow_zero_in_degree(self, set_value):
        self._allow_zero_in_degree = set_value

    def forward(self, graph, feat, get_attention=False):
        h_src, h_dst, one = _rows("DotGatConv", graph, feat, self._allow_zero_in_degree)
        H, D = self._num_heads, self._out_feats
        n_dst = graph.number_of_dst_nodes()
        kv = ops.linear(h_src, self.fc.weight).view(-1, H, D)
        if one:
            q = kv[:n_dst] if _sampled(graph) else kv
        else:
            q = ops.linear(h_dst, self.fc.weight).view(-1, H, D)
        return ops.dot_attention(graph, q, kv, kv, D ** -0.5, return_attention=get_attention)

    def extra_repr(self):
        return f"in={self._in_src_feats}, out={self._out_feats}, heads={self._num_heads}"


class TransformerConv(nn.Module):
    """Graph transformer layer (PyG's `TransformerConv`; Shi et al., arXiv:2009.03509), parameter names as PyG's:

        q = lin_query(x_dst),  k = lin_key(x_src),  v = lin_value(x_src)         [n, H, C]
        a = softmax over the in-edges of (q . k) / sqrt(C), dropout(a);   out[v] = sum_u a * v[u]   -> [n_dst, H * C], or the heads' mean [n_dst, C]
        root_weight:  x_r = lin_skip(x_dst);  beta: b = sigmoid(lin_beta([out, x_r, out - x_r])),  out = b x_r + (1 - b) out;  else out + x_r

    `in_channels`: an int or a (source, destination) pair.  Weights take torch's default Linear initialisation.  `edge_dim` (edge
    features in the attention) raises NotImplementedError here: that layer is `EdgeTransformerConv`.  `graph` / `feat` as `DotGatConv`, the zero-in-degree check included: with
    `allow_zero_in_degree=True` (this project's addition to PyG's surface) such a destination aggregates 0, as in PyG."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, beta=False, dropout=0.0, edge_dim=None, bias=True, root_weight=True,
                 allow_zero_in_degree=False):
        super().__init__()
        if edge_dim is not None:
            raise NotImplementedError("TransformerConv: edge features in the attention (edge_dim) are not implemented by this class; "
                                      "use EdgeTransformerConv")
        self.in_channels, self.out_channels, self.heads, self.concat = in_channels, out_channels, heads, concat
        self.beta, self.dropout, self.root_weight = beta and root_weight, float(dropout), root_weight
        self._allow_zero_in_degree = allow_zero_in_degree
        fin_src, fin_dst = _pair(tuple(in_channels) if isinstance(in_channels, list) else in_channels)
        HC = heads * out_channels
        self.lin_key = nn.Linear(fin_src, HC, bias=bias)
        self.lin_query = nn.Linear(fin_dst, HC, bias=bias)
        self.lin_value = nn.Linear(fin_src, HC, bias=bias)
        width = HC if concat else out_channels
        self.lin_skip = nn.Linear(fin_dst, width, bias=bias) if root_weight else None
        self.lin_beta = nn.Linear(3 * width, 1, bias=False) if self.beta else None

    def reset_parameters(self):
        for lin in (self.lin_key, self.lin_query, self.lin_value, self.lin_skip, self.lin_beta):
            if lin is not None:
                lin.reset_parameters()

    def _qkv(self, graph, feat):
        """The projected rows of a call: (q [n_dst, H, C], k, v [n_src, H, C], x_dst)."""
        x_src, x_dst, _ = _rows(type(self).__name__, graph, feat, self._allow_zero_in_degree)
        H, C = self.heads, self.out_channels
        lin = lambda x, fc: ops.linear(x, fc.weight, fc.bias).view(-1, H, C)
        return lin(x_dst, self.lin_query), lin(x_src, self.lin_key), lin(x_src, self.lin_value), x_dst

    def _finish(self, out, x_dst, get_attention):
        """What follows the attention: the heads' concatenation or mean, the skip term and the gate."""
        H, C = self.heads, self.out_channels
        a = None
        if get_attention:
            out, a = out
        out = out.reshape(-1, H * C) if self.concat else (out.view(-1, C) if H == 1 else out.mean(1))
        if self.root_weight:
            x_r = ops.linear(x_dst, self.lin_skip.weight, self.lin_skip.bias)
            if self.lin_beta is not None:
                b = torch.sigmoid(ops.linear(torch.cat([out, x_r, out - x_r], dim=-1), self.lin_beta.weight))
                out = b * x_r + (1 - b) * out
            else:
                out = out + x_r
        return (out, a) if get_attention else out

    def forward(self, graph, feat, get_attention=False):
        q, k, v, x_dst = self._qkv(graph, feat)
        out = ops.dot_attention(graph, q, k, v, self.out_channels ** -0.5, p=self.dropout if self.training else 0.0,
                                return_attention=get_attention)
        return self._finish(out, x_dst, get_attention)

    def extra_repr(self):
        return f"{self.in_channels}, {self.out_channels}, heads={self.heads}, concat={self.concat}, beta={self.beta}, root_weight={self.root_weight}"


class EdgeTransformerConv(TransformerConv):
    """`TransformerConv` with K raw edge features in the attention (PyG's `TransformerConv(edge_dim=K)`, whose parameter names and
    `state_dict` keys it has): `lin_edge = nn.Linear(edge_dim, heads * out_channels, bias=False)` and, for the edge e = u -> v,

        E_e = lin_edge(edge_attr[e]).view(H, C);   a = softmax of (q[v] . (k[u] + E_e)) / sqrt(C), dropout(a);   out[v] = sum_e a (v[u] + E_e)

    the rest as `TransformerConv`.  `forward(graph, feat, edge_attr, get_attention=False)`: `edge_attr` float32 [E, edge_dim] in edge-id
    order (on a Block or Subgraph: its own edges' rows).  The attention is `ops.dot_attention_edge`: on the GPU the encoder stays
    outside the sweep, which reads an edge's K raw floats (K <= 16, C >= K; else the tensor form).  A class of its own because
    `TransformerConv(edge_dim=)` keeps refusing."""

    def __init__(self, in_channels, out_channels, heads=1, concat=True, beta=False, dropout=0.0, edge_dim=None, bias=True, root_weight=True,
                 allow_zero_in_degree=False):
        if edge_dim is None or int(edge_dim) < 1:
            raise ValueError(f"EdgeTransformerConv: edge_dim must be at least 1, got {edge_dim}")
        super().__init__(in_channels, out_channels, heads, concat, beta, dropout, None, bias, root_weight, allow_zero_in_degree)
        self.edge_dim = int(edge_dim)
        self.lin_edge = nn.Linear(self.edge_dim, heads * out_channels, bias=False)

    def reset_parameters(self):
        super().reset_parameters()
        self.lin_edge.reset_parameters()

    def forward(self, graph, feat, edge_attr, get_attention=False):
        E = graph.number_of_edges()
        if edge_attr is None or edge_attr.dim() != 2 or tuple(edge_attr.shape) != (E, self.edge_dim):
            raise ValueError(f"edge_attr must be [{E}, {self.edge_dim}] (one row of raw features per edge, edge-id order), got "
                             f"{None if edge_attr is None else tuple(edge_attr.shape)}")
        q, k, v, x_dst = self._qkv(graph, feat)
        out = ops.dot_attention_edge(graph, q, k, v, edge_attr, self.lin_edge.weight, self.out_channels ** -0.5,
                                     p=self.dropout if self.training else 0.0, return_attention=get_attention)
        return self._finish(out, x_dst, get_attention)

    def extra_repr(self):
        return super().extra_repr() + f", edge_dim={self.edge_dim}"


class UniMP(nn.Module):
    """UniMP's graph transformer stack (Shi et al., arXiv:2009.03509) in `nn.GATv2`'s shape: n_layers `TransformerConv` with the gated
    residual (`beta`), the hidden ones with `n_heads` heads of `n_hidden` concatenated, the output layer's heads of `n_classes` averaged;
    `dropout(activation(norm(h)))` between them (BatchNorm1d with norm="batch": the fused epilogue - the paper's LayerNorm is not
    built), nothing after the last.  The labels-as-input with a random mask of the paper is `train.train_step(use_labels=True,
    mask_rate=...)`: `in_feats` then counts the label columns.  `forward` has `GCN.forward`'s contract; `edge_weight` raises ValueError, and so
    does `edge_feats`: the stack with edge features is `EdgeUniMP`."""

    def __init__(self, in_feats, n_classes, n_hidden, n_layers, n_heads, activation, norm="none", dropout=0.0, input_drop=0.0,
                 attn_drop=0.0, beta=True):
        super().__init__()
        self._build(in_feats, n_classes, n_hidden, n_layers, n_heads, activation, norm, dropout, input_drop, attn_drop, beta, None)

    def _build(self, in_feats, n_classes, n_hidden, n_layers, n_heads, activation, norm, dropout, input_drop, attn_drop, beta, edge_dim):
        if norm not in ("none", "batch"):
            raise ValueError(f'norm must be "none" or "batch", got {norm!r}')
        self.n_layers, self.n_hidden, self.n_classes, self.num_heads = n_layers, n_hidden, n_classes, n_heads
        self.edge_dim = edge_dim
        edge = {} if edge_dim is None else dict(edge_dim=edge_dim)
        self.convs, self.norms = nn.ModuleList(), nn.ModuleList()
        for i in range(n_layers):
            last = i == n_layers - 1
            fin = n_heads * n_hidden if i > 0 else in_feats
            conv = TransformerConv if edge_dim is None else EdgeTransformerConv
            self.convs.append(conv(fin, n_classes if last else n_hidden, n_heads, concat=not last, beta=beta, dropout=attn_drop,
                                   allow_zero_in_degree=True, **edge))         # sampled blocks have such rows: they keep their skip term
            if not last and norm == "batch":
                self.norms.append(nn.BatchNorm1d(n_heads * n_hidden))
        self.input_drop, self.dropout = nn.Dropout(input_drop), nn.Dropout(dropout)
        self.activation = activation

    def forward(self, graph, feat=None, edge_weight=None, edge_feats=None):
        """`graph`: a Graph (`feat` in original node order), or a list of n_layers sampled blocks: layer i runs on blocks[i], `feat`
        defaults to blocks[0].srcdata["feat"].  `edge_feats` (with `edge_dim`; raw [E, edge_dim] in edge-id order), as
        `DeeperGCN.forward` takes it: for a Graph or Subgraph a tensor, an `edata` key or None for edata["feat"]; for a block list a
        list of one tensor per block, or None for each block's rows of the parent's edata["feat"]."""
        if edge_weight is not None:
            raise ValueError("edge_weight is for the GCN stacks: a UniMP stack learns its edge weights")
        blocks = _block_list(graph, feat, self.n_layers)
        efs = layer_edge_feats(type(self).__name__, self.edge_dim, self.n_layers, graph, blocks, edge_feats)
        h = graph.to_internal(feat) if blocks is None else (blocks[0].srcdata["feat"] if feat is None else feat)
        h = self.input_drop(h)
        for i in range(self.n_layers):
            g = graph if blocks is None else blocks[i]
            h = self.convs[i](g, h) if efs[i] is None else self.convs[i](g, h, efs[i])
            if i < self.n_layers - 1:
                if len(self.norms):
                    h = _epilogue(h, self.norms[i], self.activation, self.dropout, self.training)
                else:
                    h = self.dropout(self.activation(h))
        return h if blocks is not None else graph.to_original(h)


class EdgeUniMP(UniMP):
    """`UniMP` on a graph with K raw features per edge (`edge_dim=K`; the published ogbn-proteins model): every layer is an
    `EdgeTransformerConv` with its own `lin_edge`, and `forward` hands each layer the raw edge features of its graph, by default the
    column edata["feat"].  The other arguments, modules and keys are `UniMP`'s.  A class of its own, as `EdgeTransformerConv` is:
    `UniMP`'s constructor keeps its parameter list."""

    def __init__(self, in_feats, n_classes, n_hidden, n_layers, n_heads, activation, norm="none", dropout=0.0, input_drop=0.0,
                 attn_drop=0.0, beta=True, edge_dim=None):
        nn.Module.__init__(self)           # (not UniMP.__init__, which would build the stack without lin_edge first)
        if edge_dim is None or int(edge_dim) < 1:
            raise ValueError(f"EdgeUniMP: edge_dim must be at least 1, got {edge_dim}")
        self._build(in_feats, n_classes, n_hidden, n_layers, n_heads, activation, norm, dropout, input_drop, attn_drop, beta, int(edge_dim))
