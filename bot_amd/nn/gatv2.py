"""GATv2 (Brody, Alon, Yahav, "How Attentive are Graph Attention Networks?", ICLR 2022): `GATv2Conv` with the surface of DGL's
`dgl.nn.GATv2Conv` where DESIGN §1 states it, and the `GATv2` stack in `nn.GraphSAGE`'s shape.

The score a . leaky_relu(W_l h_u + W_r h_v) has its nonlinearity inside the dot product, so - unlike `GATConv`'s - it does not split into
one scalar per node and head: the logits come from `ops.gatv2_logits` (csrc/gatv2.hip), one sweep that gathers the source row and
reduces over each head's columns on the fly.  Everything behind the logits is the GAT path's: the edge softmax over given logits
(`ops.gat_attention(ee=...)`), dropout on the weights, the weighted sweep (`ops.u_mul_e_sum`), the residual.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops
from ..errors import DGLError
from . import _block_list, _epilogue, _pair, _sampled, _src_rows, has_zero_in_degree

__all__ = ["GATv2Conv", "GATv2"]


class GATv2Conv(nn.Module):
    """GATv2 layer (DGL's `GATv2Conv`):

        fs = fc_src(h_src),  fd = fc_dst(h_dst)                                  [n, H, D]
        e  = attn . leaky_relu(fs[u] + fd[v])  per edge u -> v and head;   a = softmax of e over the in-edges of v
        rst[v] = sum_u a * fs[u]  (+ res_fc(h_dst))  -> activation               [n_dst, H, D]

    `fc_dst` is `fc_src` under `share_weights`; `res_fc` (with `residual`) is a bias-free Linear when in_dst != H * D, else the identity.
    `graph`: a whole Graph, a Subgraph or a sampled Block (destinations = the first n_dst source rows); `feat`: a tensor or a
    (feat_src, feat_dst) pair.  A partition with a halo plan raises ValueError."""

    def __init__(self, in_feats, out_feats, num_heads, feat_drop=0.0, attn_drop=0.0, negative_slope=0.2, residual=False, activation=None,
                 allow_zero_in_degree=False, bias=True, share_weights=False):
        super().__init__()
        self._num_heads, self._out_feats = num_heads, out_feats
        self._in_src_feats, self._in_dst_feats = _pair(tuple(in_feats) if isinstance(in_feats, list) else in_feats)
        self._allow_zero_in_degree, self.share_weights = allow_zero_in_degree, share_weights
        if share_weights and self._in_src_feats != self._in_dst_feats:
            raise DGLError(f"share_weights needs equal source and destination widths, got {self._in_src_feats} and {self._in_dst_feats}")
        self.fc_src = nn.Linear(self._in_src_feats, out_feats * num_heads, bias=bias)
        self.fc_dst = self.fc_src if share_weights else nn.Linear(self._in_dst_feats, out_feats * num_heads, bias=bias)
        self.attn = nn.Parameter(torch.empty(1, num_heads, out_feats))
        self.feat_drop, self.attn_drop = nn.Dropout(feat_drop), nn.Dropout(attn_drop)
        self.negative_slope = float(negative_slope)
        if residual:
            self.res_fc = (nn.Linear(self._in_dst_feats, num_heads * out_feats, bias=False) if self._in_dst_feats != num_heads * out_feats
                           else nn.Identity())
        else:
            self.register_buffer("res_fc", None)
        self.activation = activation
        self.reset_parameters()

    def reset_parameters(self):
        gain = nn.init.calculate_gain("relu")
        for lin in (self.fc_src, self.fc_dst, self.res_fc):
            if isinstance(lin, nn.Linear):
                nn.init.xavier_normal_(lin.weight, gain=gain)
                if lin.bias is not None:
                    nn.init.zeros_(lin.bias)
        nn.init.xavier_normal_(self.attn, gain=gain)

    def set_allow_zero_in_degree(self, set_value):
        self._allow_zero_in_degree = set_value

    def forward(self, graph, feat, get_attention=False):
        if graph.halo is not None:
            raise ValueError("GATv2Conv on a partitioned graph (a halo plan) is not supported: it takes whole graphs, Subgraphs and "
                             "sampled blocks")
        if not self._allow_zero_in_degree and has_zero_in_degree(graph):
            raise DGLError(
                "There are 0-in-degree nodes in the graph, output for those nodes will be invalid. "
                "Adding self-loop on the input graph by calling `g = g.add_self_loop()` will resolve the issue. "
                "Setting ``allow_zero_in_degree`` to be `True` when constructing this module will suppress the check.")
        H, D = self._num_heads, self._out_feats
        n_dst = graph.number_of_dst_nodes()
        lin = lambda x, fc: ops.linear(x, fc.weight, fc.bias)
        if isinstance(feat, tuple):
            h_src, h_dst = _src_rows(graph, self.feat_drop(feat[0])), self.feat_drop(feat[1])
            if h_dst.shape[0] != n_dst:
                raise ValueError(f"feat_dst holds {h_dst.shape[0]} rows, the graph has {n_dst} destination nodes")
            fs, fd = lin(h_src, self.fc_src), lin(h_dst, self.fc_dst)
        else:
            h_src = _src_rows(graph, self.feat_drop(feat))
            h_dst = h_src[:n_dst] if _sampled(graph) else h_src      # a block's destinations are its first n_dst sources
            fs = lin(h_src, self.fc_src)
            if self.share_weights:
                fd = fs[:n_dst] if _sampled(graph) else fs
            else:
                fd = lin(h_dst, self.fc_dst)
        fs, fd = fs.view(-1, H, D), fd.view(-1, H, D)
        e = ops.gatv2_logits(graph, fs, fd, self.attn, self.negative_slope, order="csc")
        a = ops.gat_attention(graph, None, None, e, negative_slope=1.0, order="csc", ee_order="csc")     # the edge softmax of e
        rst = ops.u_mul_e_sum(graph, fs, self.attn_drop(a), order="csc")
        if self.res_fc is not None:
            res = h_dst if isinstance(self.res_fc, nn.Identity) else ops.linear(h_dst, self.res_fc.weight)
            rst = rst + res.view(-1, H, D)
        if self.activation is not None:
            rst = self.activation(rst)
        return (rst, a) if get_attention else rst

    def extra_repr(self):
        return (f"in=({self._in_src_feats}, {self._in_dst_feats}), out={self._out_feats}, heads={self._num_heads}, "
                f"share_weights={self.share_weights}")


class GATv2(nn.Module):
    """GATv2 stack in `nn.GraphSAGE`'s shape: n_layers GATv2Conv, the hidden ones with `n_heads` heads of `n_hidden` flattened, the
    output layer's `n_out_heads` heads of `n_classes` averaged; `dropout(activation(norm(h)))` between them (BatchNorm1d with
    norm="batch": the fused epilogue), nothing after the last.  `forward` has `GCN.forward`'s contract, so the stack runs under
    train.train_step, minibatch.train_epoch, minibatch.subgraph_step and train_epoch_subgraphs unchanged; it learns its edge weights
    and takes none (`edge_weight` raises ValueError)."""

    def __init__(self, in_feats, n_classes, n_hidden, n_layers, n_heads, activation, norm="none", dropout=0.0, input_drop=0.0,
                 attn_drop=0.0, negative_slope=0.2, residual=False, share_weights=False, n_out_heads=1, allow_zero_in_degree=False):
        super().__init__()
        if norm not in ("none", "batch"):
            raise ValueError(f'norm must be "none" or "batch", got {norm!r}')
        self.n_layers, self.n_hidden, self.n_classes, self.num_heads = n_layers, n_hidden, n_classes, n_heads
        self.convs, self.norms = nn.ModuleList(), nn.ModuleList()
        for i in range(n_layers):
            last = i == n_layers - 1
            fin = n_heads * n_hidden if i > 0 else in_feats
            self.convs.append(GATv2Conv(fin, n_classes if last else n_hidden, n_out_heads if last else n_heads, attn_drop=attn_drop,
                                        negative_slope=negative_slope, residual=residual, bias=norm == "none" or last,
                                        share_weights=share_weights, allow_zero_in_degree=allow_zero_in_degree))
            if not last and norm == "batch":
                self.norms.append(nn.BatchNorm1d(n_heads * n_hidden))
        self.input_drop, self.dropout = nn.Dropout(input_drop), nn.Dropout(dropout)
        self.activation = activation

    def forward(self, graph, feat=None, edge_weight=None):
        """`graph`: a Graph (`feat` in original node order), or a list of n_layers sampled blocks: layer i runs on blocks[i], `feat`
        defaults to blocks[0].srcdata["feat"]."""
        if edge_weight is not None:
            raise ValueError("edge_weight is for the GCN stacks: a GATv2 stack learns its edge weights")
        blocks = _block_list(graph, feat, self.n_layers)
        h = graph.to_internal(feat) if blocks is None else (blocks[0].srcdata["feat"] if feat is None else feat)
        h = self.input_drop(h)
        for i in range(self.n_layers):
            h = self.convs[i](graph if blocks is None else blocks[i], h)
            if i < self.n_layers - 1:
                h = h.flatten(1)
                if len(self.norms):
                    h = _epilogue(h, self.norms[i], self.activation, self.dropout, self.training)
                else:
                    h = self.dropout(self.activation(h))
        # (one output head: the mean over it is the head itself, bit for bit - a view, not a reduction launch and its backward)
        h = h.view(h.shape[0], -1) if h.shape[1] == 1 else h.mean(1)
        return h if blocks is not None else graph.to_original(h)
