"""GatedGCN with an edge stream (Bresson & Laurent, "Residual Gated Graph ConvNets", arXiv:1711.07553, in the form of Dwivedi et al.,
"Benchmarking Graph Neural Networks", arXiv:2003.00982, and of GraphGPS's local layer): `GatedGCNConv` with the surface and parameter
names of DGL's layer of that name, and the `GatedGCN` node-classification stack of the benchmark.

The gate's pre-activation e_hat = D h_u + E h_v + C e has a per-edge term and is itself the layer's second output, which the next layer
reads: [E, F] is the model's state here.  The aggregation is `ops.gated_edge_sum` (csrc/spmm_gate_edge.hip): one sweep that gathers the
neighbour's D and B rows - the two column blocks of ONE merged projection - streams the edge's C row at the walk's own position, stores
e_hat and forms the gate on the fly; the backward forms the gates again from the stored e_hat.  Nothing else of size [E, F] exists in
the aggregation (the stream's BatchNorm, residual and dropout are dense passes over it).
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from . import _sampled, _src_rows
from .gated import _BiasedBlocks

__all__ = ["GatedGCNConv", "GatedGCN"]


def _lin(x, lin):
    return ops.linear(x, lin.weight, lin.bias) if x.is_cuda else F.linear(x, lin.weight, lin.bias)


class GatedGCNConv(nn.Module):
    """DGL's `GatedGCNConv`:

        e_hat[u -> v] = D(h_u) + E(h_v) + C(e[u -> v])
        h_new[v]      = A(h_v) + sum_u sigmoid(e_hat) * B(h_u) / (sum_u sigmoid(e_hat) + 1e-6)

    then, for each of the two streams, BatchNorm, activation, the residual add and dropout, in that order.  Parameters: `A`, `B`, `D`,
    `E` = nn.Linear(input_feats, output_feats), `C` = nn.Linear(edge_feats, output_feats), `bn_node`, `bn_edge` = BatchNorm1d.  The
    residual is off for both streams unless input_feats == edge_feats == output_feats.  D and B run as ONE projection of width
    2 * output_feats.  `graph`: a whole Graph, a Subgraph or a sampled Block; `feat`: a tensor or a (feat_src, feat_dst) pair; `edge_feat`:
    [E, edge_feats] in edge-id order (`order="eid"`) or CSC position order (`order="csc"`, what a stack keeps between its layers: no
    permutation); the returned e is in the same order, or None with `edge_out=False` (the last layer of a node-level net: the edge
    stream's epilogue is skipped and, without gradients, nothing per edge is written).  A halo plan raises ValueError."""

    def __init__(self, input_feats, edge_feats, output_feats, dropout=0.0, batch_norm=True, residual=True, activation=F.relu):
        super().__init__()
        self._in, self._edge, self._out = int(input_feats), int(edge_feats), int(output_feats)
        self.dropout = nn.Dropout(dropout)
        self.batch_norm = bool(batch_norm)
        self.activation = activation
        self.residual = bool(residual) and self._in == self._edge == self._out
        self.A = nn.Linear(input_feats, output_feats)
        self.B = nn.Linear(input_feats, output_feats)
        self.C = nn.Linear(edge_feats, output_feats)
        self.D = nn.Linear(input_feats, output_feats)
        self.E = nn.Linear(input_feats, output_feats)
        self.bn_node = nn.BatchNorm1d(output_feats)
        self.bn_edge = nn.BatchNorm1d(output_feats)

    def reset_parameters(self):
        for m in (self.A, self.B, self.C, self.D, self.E, self.bn_node, self.bn_edge):
            m.reset_parameters()

    def _gate_value(self, h_src):
        """(q, v) = (D h, B h): the two column blocks of one projection of width 2 * output_feats, biases added in the packing pass."""
        Fo = self._out
        w = torch.cat((self.D.weight, self.B.weight))
        pieces = None
        if h_src.is_cuda:
            from .. import gemm
            pieces = gemm.linear_blocks(h_src, w, [Fo, Fo])
        if pieces is None:
            y = ops.linear(h_src, w) if h_src.is_cuda else F.linear(h_src, w)
            pieces = torch.split(y, [Fo, Fo], dim=1)
        return _BiasedBlocks.apply(pieces[0], pieces[1], self.D.bias, self.B.bias)

    def _stream(self, x, bn, x_in):
        """BatchNorm, activation, residual add, dropout - the first two as the fused pass where it applies (any 2-D matrix: the edge
        stream has E rows)."""
        act = self.activation
        if self.batch_norm:
            if x.is_cuda and x.dtype == torch.float32:
                relu = act in (F.relu, torch.relu)
                x = ops.bn_relu_dropout(x.contiguous(), bn, relu=relu, p=0.0, training=self.training)
                act = None if relu else act
            else:
                x = bn(x)
        if act is not None:
            x = act(x)
        if self.residual:
            x = x_in + x
        return self.dropout(x)

    def forward(self, graph, feat, edge_feat, order="eid", edge_out=True):
        if graph.halo is not None:
            raise ValueError("GatedGCNConv on a partitioned graph (a halo plan) is not supported: it takes whole graphs, Subgraphs and "
                             "sampled blocks")
        n_dst = graph.number_of_dst_nodes()
        if isinstance(feat, tuple):
            h_src, h_dst = _src_rows(graph, feat[0]), feat[1]
            if h_dst.shape[0] != n_dst:
                raise ValueError(f"feat_dst holds {h_dst.shape[0]} rows, the graph has {n_dst} destination nodes")
        else:
            h_src = _src_rows(graph, feat)
            h_dst = h_src[:n_dst] if _sampled(graph) else h_src      # a block's destinations are its first n_dst sources
        if edge_feat.dim() != 2 or edge_feat.shape[0] != graph.number_of_edges():
            raise ValueError(f"edge_feat must be [{graph.number_of_edges()}, {self._edge}] (one row per edge), got {tuple(edge_feat.shape)}")
        k = _lin(h_dst, self.E)
        q, v = self._gate_value(h_src)
        c = _lin(edge_feat, self.C)
        agg, e = ops.gated_edge_sum(graph, k, q, v, c, normalize=True, eps=1e-6, order=order, want_edge=edge_out)
        h = self._stream(_lin(h_dst, self.A) + agg, self.bn_node, h_dst)
        if e is not None:
            e = self._stream(e, self.bn_edge, edge_feat)
        return h, e

    def extra_repr(self):
        return f"in={self._in}, edge={self._edge}, out={self._out}, batch_norm={self.batch_norm}, residual={self.residual}"


class GatedGCN(nn.Module):
    """The benchmark's node-classification net: `embedding_h` and `embedding_e` (Linear), n_layers `GatedGCNConv` of n_hidden, an output
    Linear.  The raw edge features are permuted to CSC position order ONCE (cached per graph and tensor identity / version) and the edge
    stream stays in position order through all layers; the last layer runs with edge_out=False.  Mini-batches are cluster and
    GraphSAINT `Subgraph`s (`minibatch.subgraph_step(..., node_loss=...)`); a list of sampled blocks raises ValueError: each block has
    its own edges, so an edge stream cannot pass from one to the next."""

    def __init__(self, in_feats, edge_in_feats, n_classes, n_hidden, n_layers, dropout=0.0, input_drop=0.0, batch_norm=True, residual=True):
        super().__init__()
        self.n_layers, self.n_hidden, self.n_classes = n_layers, n_hidden, n_classes
        self.embedding_h = nn.Linear(in_feats, n_hidden)
        self.embedding_e = nn.Linear(edge_in_feats, n_hidden)
        self.convs = nn.ModuleList(GatedGCNConv(n_hidden, n_hidden, n_hidden, dropout, batch_norm, residual) for _ in range(n_layers))
        self.out = nn.Linear(n_hidden, n_classes)
        self.input_drop = nn.Dropout(input_drop)

    def edge_rows(self, graph, edge_feats=None):
        """The raw edge features in CSC position order: a tensor in edge-id order, an `edata` key, or None for edata["feat"]."""
        key = "feat" if edge_feats is None else edge_feats
        ef = graph.edata[key] if isinstance(key, str) else key
        if ef.dim() != 2 or ef.shape[0] != graph.number_of_edges():
            raise ValueError(f"edge_feats must be [{graph.number_of_edges()}, K] (one row per edge), got {tuple(ef.shape)}")
        return ef if ops._csc_edge_rows(graph) is None else ops.edge_features_csc(graph, ef)

    def forward(self, graph, feat=None, edge_feats=None):
        if isinstance(graph, (list, tuple)):
            raise ValueError("GatedGCN takes a Graph or a Subgraph, not a list of sampled blocks: each block has its own edges, so the edge "
                             "stream cannot pass from one block to the next (mini-batches: cluster or GraphSAINT subgraphs)")
        if graph.halo is not None:
            raise ValueError("GatedGCN on a partitioned graph (a halo plan) is not supported")
        h = graph.to_internal(graph.ndata["feat"] if feat is None else feat)
        e = _lin(self.edge_rows(graph, edge_feats), self.embedding_e)
        h = _lin(self.input_drop(h), self.embedding_h)
        for i, conv in enumerate(self.convs):
            h, e = conv(graph, h, e, order="csc", edge_out=i < self.n_layers - 1)
        return graph.to_original(_lin(h, self.out))
