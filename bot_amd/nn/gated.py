"""Residual gated graph convolution (Bresson & Laurent, "Residual Gated Graph ConvNets", arXiv:1711.07553; the GatedGCN of Dwivedi et
al., "Benchmarking Graph Neural Networks", arXiv:2003.00982, and of GraphGPS): `ResGatedGraphConv` with the surface of PyG's layer of
that name where DESIGN §1 states it, and the `ResGatedGCN` stack in `nn.GraphSAGE`'s shape.

Every edge carries a sigmoid gate PER CHANNEL computed from both endpoints, sigmoid(lin_key(h_v) + lin_query(h_u)), so the weight of a
neighbour's row is a vector that splits neither into per-node scalars (the GAT trick) nor into a source-only message (GENConv's).  The
aggregation is `ops.gated_sum` (csrc/spmm_gate.hip): one sweep that gathers the neighbour's query and value rows - the two column blocks
of ONE merged projection, so one contiguous row - and forms the gate on the fly; nothing of size [E, F] exists in either pass.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..errors import DGLError
from . import _block_list, _epilogue, _pair, _sampled, _src_rows, has_zero_in_degree

__all__ = ["ResGatedGraphConv", "ResGatedGCN"]


class _BiasedBlocks(torch.autograd.Function):
    """(q + bq, v + bv) written side by side into ONE [n, 2F] buffer and returned as its two column blocks: the projection's blocks get
    their biases in the pass that packs them, so a neighbour's gate row and value row stay one contiguous gathered row for the sweeps.
    The bias gradients are column sums (on the GPU by the column-statistics kernel, as `ops.add_bias`)."""

    @staticmethod
    def forward(ctx, q, v, bq, bv):
        Fo = q.shape[1]
        buf = torch.empty((q.shape[0], 2 * Fo), dtype=q.dtype, device=q.device)
        torch.add(q, bq, out=buf[:, :Fo])
        torch.add(v, bv, out=buf[:, Fo:])
        return buf[:, :Fo], buf[:, Fo:]

    @staticmethod
    def backward(ctx, dq, dv):
        from .. import _C
        colsum = (lambda d: _C.colsum(d.contiguous())) if dq.is_cuda and dq.dtype == torch.float32 else (lambda d: d.sum(0))
        return dq, dv, colsum(dq) if ctx.needs_input_grad[2] else None, colsum(dv) if ctx.needs_input_grad[3] else None


class ResGatedGraphConv(nn.Module):
    """Residual gated graph convolution (PyG's `ResGatedGraphConv` without edge features):

        out[v] = lin_skip(h_v) + sum over the in-edges u -> v of sigmoid(lin_key(h_v) + lin_query(h_u)) * lin_value(h_u)  (+ bias)

    `normalize=True` is GatedGCN's form, the sum divided per channel by (the sum of the gates + eps).  Parameters carry PyG's names:
    `lin_key` (destination side), `lin_query`, `lin_value` (source side), all with a bias; `lin_skip` (bias-free, with `root_weight`);
    `bias`.  Query and value run as ONE projection of width 2 * out_feats on the concatenated weight.  `graph`: a whole Graph, a Subgraph
    or a sampled Block (destinations = the first n_dst source rows); `feat`: a tensor or a (feat_src, feat_dst) pair.  A partition with a
    halo plan raises ValueError."""

    def __init__(self, in_feats, out_feats, normalize=False, eps=1e-6, root_weight=True, bias=True, feat_drop=0.0, activation=None,
                 allow_zero_in_degree=True):
        super().__init__()
        self._in_src_feats, self._in_dst_feats = _pair(tuple(in_feats) if isinstance(in_feats, list) else in_feats)
        self._out_feats, self.normalize, self.eps, self.root_weight = out_feats, bool(normalize), float(eps), bool(root_weight)
        self._allow_zero_in_degree = allow_zero_in_degree
        self.lin_key = nn.Linear(self._in_dst_feats, out_feats)
        self.lin_query = nn.Linear(self._in_src_feats, out_feats)
        self.lin_value = nn.Linear(self._in_src_feats, out_feats)
        if root_weight:
            self.lin_skip = nn.Linear(self._in_dst_feats, out_feats, bias=False)
        else:
            self.register_module("lin_skip", None)
        if bias:
            self.bias = nn.Parameter(torch.zeros(out_feats))
        else:
            self.register_parameter("bias", None)
        self.feat_drop = nn.Dropout(feat_drop)
        self.activation = activation

    def reset_parameters(self):
        for lin in (self.lin_key, self.lin_query, self.lin_value, self.lin_skip):
            if lin is not None:
                lin.reset_parameters()
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def set_allow_zero_in_degree(self, set_value):
        self._allow_zero_in_degree = set_value

    def _query_value(self, h_src):
        """(q, v): the two column blocks of one projection of width 2 * out_feats."""
        Fo = self._out_feats
        w = torch.cat((self.lin_query.weight, self.lin_value.weight))
        pieces = None
        if h_src.is_cuda:
            from .. import gemm
            pieces = gemm.linear_blocks(h_src, w, [Fo, Fo])        # halves path: the blocks' gradients never meet in a `cat`
        if pieces is None:
            y = ops.linear(h_src, w) if h_src.is_cuda else F.linear(h_src, w)
            pieces = torch.split(y, [Fo, Fo], dim=1)
        return _BiasedBlocks.apply(pieces[0], pieces[1], self.lin_query.bias, self.lin_value.bias)

    def forward(self, graph, feat):
        if graph.halo is not None:
            raise ValueError("ResGatedGraphConv on a partitioned graph (a halo plan) is not supported: it takes whole graphs, Subgraphs and "
                             "sampled blocks")
        if not self._allow_zero_in_degree and has_zero_in_degree(graph):
            raise DGLError(
                "There are 0-in-degree nodes in the graph, output for those nodes will be invalid. "
                "Adding self-loop on the input graph by calling `g = g.add_self_loop()` will resolve the issue. "
                "Setting ``allow_zero_in_degree`` to be `True` when constructing this module will suppress the check.")
        n_dst = graph.number_of_dst_nodes()
        if isinstance(feat, tuple):
            h_src, h_dst = _src_rows(graph, self.feat_drop(feat[0])), self.feat_drop(feat[1])
            if h_dst.shape[0] != n_dst:
                raise ValueError(f"feat_dst holds {h_dst.shape[0]} rows, the graph has {n_dst} destination nodes")
        else:
            h_src = _src_rows(graph, self.feat_drop(feat))
            h_dst = h_src[:n_dst] if _sampled(graph) else h_src      # a block's destinations are its first n_dst sources
        lin = (lambda x, w, b=None: ops.linear(x, w, b)) if h_src.is_cuda else F.linear
        k = lin(h_dst, self.lin_key.weight, self.lin_key.bias)
        q, v = self._query_value(h_src)
        rst = ops.gated_sum(graph, k, q, v, normalize=self.normalize, eps=self.eps)
        if self.lin_skip is not None:
            rst = rst + lin(h_dst, self.lin_skip.weight)
        if self.bias is not None:
            rst = rst + self.bias
        if self.activation is not None:
            rst = self.activation(rst)
        return rst

    def extra_repr(self):
        return (f"in=({self._in_src_feats}, {self._in_dst_feats}), out={self._out_feats}, normalize={self.normalize}, "
                f"root_weight={self.root_weight}")


class ResGatedGCN(nn.Module):
    """Gated stack in `nn.GraphSAGE`'s shape: n_layers ResGatedGraphConv, `dropout(activation(norm(h)))` between them (BatchNorm1d with
    norm="batch": the fused epilogue), nothing after the last.  `forward` has `GCN.forward`'s contract, so the stack runs under
    train.train_step, minibatch.train_epoch, minibatch.subgraph_step and train_epoch_subgraphs unchanged; it learns its gates and takes
    no edge weights (`edge_weight` raises ValueError)."""

    def __init__(self, in_feats, n_classes, n_hidden, n_layers, activation, norm="none", dropout=0.0, input_drop=0.0, normalize=False,
                 eps=1e-6, root_weight=True, allow_zero_in_degree=True):
        super().__init__()
        if norm not in ("none", "batch"):
            raise ValueError(f'norm must be "none" or "batch", got {norm!r}')
        self.n_layers, self.n_hidden, self.n_classes = n_layers, n_hidden, n_classes
        self.convs, self.norms = nn.ModuleList(), nn.ModuleList()
        for i in range(n_layers):
            last = i == n_layers - 1
            fout = n_classes if last else n_hidden
            self.convs.append(ResGatedGraphConv(n_hidden if i > 0 else in_feats, fout, normalize=normalize, eps=eps, root_weight=root_weight,
                                                bias=norm == "none" or last, allow_zero_in_degree=allow_zero_in_degree))
            if not last and norm == "batch":
                self.norms.append(nn.BatchNorm1d(fout))
        self.input_drop, self.dropout = nn.Dropout(input_drop), nn.Dropout(dropout)
        self.activation = activation

    def forward(self, graph, feat=None, edge_weight=None):
        """`graph`: a Graph (`feat` in original node order), or a list of n_layers sampled blocks: layer i runs on blocks[i], `feat`
        defaults to blocks[0].srcdata["feat"]."""
        if edge_weight is not None:
            raise ValueError("edge_weight is for the GCN stacks: a gated stack learns its gates")
        blocks = _block_list(graph, feat, self.n_layers)
        h = graph.to_internal(feat) if blocks is None else (blocks[0].srcdata["feat"] if feat is None else feat)
        h = self.input_drop(h)
        for i in range(self.n_layers):
            h = self.convs[i](graph if blocks is None else blocks[i], h)
            if i < self.n_layers - 1:
                if len(self.norms):
                    h = _epilogue(h, self.norms[i], self.activation, self.dropout, self.training)
                else:
                    h = self.dropout(self.activation(h))
        return h if blocks is not None else graph.to_original(h)
