"""GraphSAGE (Hamilton, Ying, Leskovec, NeurIPS 2017): `SAGEConv` with the mean, gcn and pool aggregators, interface-identical to
DGL 0.6's `dgl.nn.SAGEConv` where DESIGN §1 states it, and the `GraphSAGE` stack in `nn.GCN`'s shape.

mean and gcn are ONE launch of the weighted sum sweep: the divisor 1 / deg (1 / (deg + 1)) rides as a constant per-position weight - a
constant weight costs no backward - and the self term enters through the sweep's `addend` epilogue.  pool runs on the max sweep
(`ops.copy_u_max`, csrc/spmm_max.hip) with the ReLU of `relu(fc_pool(h))` folded behind the reduce.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import ops
from ..errors import DGLError
from ..graph import take_rows
from . import _block_list, _edge_weight, _epilogue, _graph_cache, _sampled, _src_rows

__all__ = ["SAGEConv", "GraphSAGE"]

AGGREGATORS = ("mean", "gcn", "pool")


def inv_degree(graph, plus_one: bool):
    """(inv [n_dst] float32, inv_pos [E, 1] float32 in CSC position order) of the structural in-degrees, once per graph:
    inv = 1 / deg (0 for a node without in-edges), or 1 / (deg + 1) with `plus_one` (the gcn aggregator counts the node itself)."""
    c = _graph_cache(graph)
    key = ("sage_inv_deg", bool(plus_one))
    if key not in c:
        deg = graph.in_degrees()
        d = deg.to(torch.float32)
        inv = 1.0 / (d + 1.0) if plus_one else torch.where(deg > 0, 1.0 / d.clamp(min=1.0), torch.zeros_like(d))
        pos = torch.repeat_interleave(inv, deg, output_size=graph.number_of_edges()).reshape(-1, 1).contiguous()
        c[key] = (inv.contiguous(), pos)
    return c[key]


def _position_order(graph, ew):
    """A caller's edge weight [E, 1] (edge-id order) in CSC position order; on a batch graph the edge id is the position."""
    from ..sampling import _BatchGraph
    return ew if isinstance(graph, _BatchGraph) else take_rows(ew, graph.csc.eid)


class SAGEConv(nn.Module):
    """GraphSAGE layer (DGL 0.6 `SAGEConv`).

        mean   fc_self(h_dst) + h_neigh,  h_neigh = mean over the in-edges of fc_neigh(h_src) when in_src > out_feats, else
               fc_neigh(mean(h_src)); a node without in-edges has mean 0
        gcn    fc_neigh((sum_in h_src + h_dst) / (in_degree + 1)), the projection in front of the sum when in_src > out_feats
        pool   fc_self(h_dst) + fc_neigh(max over the in-edges of relu(fc_pool(h_src)))

    then `activation`, then `norm`.  `graph`: a whole Graph, a Subgraph or a sampled Block (destinations = the first n_dst source rows);
    `feat`: a tensor or a (feat_src, feat_dst) pair.  `edge_weight` (float32 [E] / [E, 1], edge-id order): mean and gcn aggregate
    w_e h_u, the divisors stay the structural degrees; pool takes none (ValueError).  A partition with a halo plan raises ValueError."""

    def __init__(self, in_feats, out_feats, aggregator_type, feat_drop=0.0, bias=True, norm=None, activation=None):
        super().__init__()
        if aggregator_type == "lstm":
            raise NotImplementedError("SAGEConv: the lstm aggregator is not built (DESIGN §8); use mean, gcn or pool")
        if aggregator_type not in AGGREGATORS:
            raise DGLError(f"Invalid aggregator_type. Must be one of {set(AGGREGATORS) | {'lstm'}}. But got {aggregator_type!r} instead.")
        self._in_src_feats, self._in_dst_feats = in_feats if isinstance(in_feats, (tuple, list)) else (in_feats, in_feats)
        self._out_feats, self._aggre_type = out_feats, aggregator_type
        if aggregator_type == "gcn" and self._in_src_feats != self._in_dst_feats:
            raise DGLError(f"the gcn aggregator adds source and destination rows: their widths must agree, got "
                           f"{self._in_src_feats} and {self._in_dst_feats}")
        self.norm, self.activation = norm, activation
        self.feat_drop = nn.Dropout(feat_drop)
        if aggregator_type == "pool":
            self.fc_pool = nn.Linear(self._in_src_feats, self._in_src_feats)
        if aggregator_type != "gcn":
            self.fc_self = nn.Linear(self._in_dst_feats, out_feats, bias=bias)
        self.fc_neigh = nn.Linear(self._in_src_feats, out_feats, bias=bias)
        self.reset_parameters()

    def reset_parameters(self):
        gain = nn.init.calculate_gain("relu")
        for name in ("fc_pool", "fc_self", "fc_neigh"):
            lin = getattr(self, name, None)
            if lin is not None:
                nn.init.xavier_uniform_(lin.weight, gain=gain)

    def forward(self, graph, feat, edge_weight=None):
        if graph.halo is not None:
            raise ValueError("SAGEConv on a partitioned graph (a halo plan) is not supported: it takes whole graphs, Subgraphs and "
                             "sampled blocks")
        if isinstance(feat, tuple):
            h_src, h_dst = self.feat_drop(feat[0]), self.feat_drop(feat[1])
            paired = True
        else:
            h_src = self.feat_drop(feat)
            h_dst, paired = None, False
        h_src = _src_rows(graph, h_src)
        n_dst = graph.number_of_dst_nodes()
        prefix = lambda t: t[:n_dst] if _sampled(graph) else t      # a block's destinations are its first n_dst sources
        if not paired:
            h_dst = prefix(h_src)
        elif h_dst.shape[0] != n_dst:
            raise ValueError(f"feat_dst holds {h_dst.shape[0]} rows, the graph has {n_dst} destination nodes")
        lin = lambda x, fc: ops.linear(x, fc.weight, fc.bias)
        before = self._in_src_feats > self._out_feats                  # DGL's lin_before_mp
        kind = self._aggre_type
        if kind == "pool":
            if edge_weight is not None:
                raise ValueError("the pool aggregator takes no edge_weight: a max has no per-edge factor (DESIGN §8)")
            m = ops.copy_u_max(graph, lin(h_src, self.fc_pool), relu=True)
            rst = lin(h_dst, self.fc_self) + lin(m, self.fc_neigh)
        else:
            inv, a = inv_degree(graph, kind == "gcn")
            if edge_weight is not None:
                a = _position_order(graph, _edge_weight(graph, edge_weight)) * a
            agg = lambda x, addend: ops.u_mul_e_sum(graph, x, a, order="csc", addend=addend)
            if kind == "mean":
                if before:
                    rst = agg(lin(h_src, self.fc_neigh), lin(h_dst, self.fc_self))     # aggregate + scale + add: one launch
                else:
                    rst = lin(h_dst, self.fc_self) + lin(agg(h_src, None), self.fc_neigh)
            elif before:
                z = lin(h_src, self.fc_neigh)
                z_dst = lin(h_dst, self.fc_neigh) if paired else prefix(z)
                rst = agg(z, z_dst * inv.unsqueeze(1))
            else:
                rst = lin(agg(h_src, h_dst * inv.unsqueeze(1)), self.fc_neigh)
        if self.activation is not None:
            rst = self.activation(rst)
        if self.norm is not None:
            rst = self.norm(rst)
        return rst

    def extra_repr(self):
        return f"in=({self._in_src_feats}, {self._in_dst_feats}), out={self._out_feats}, aggregator={self._aggre_type}"


class GraphSAGE(nn.Module):
    """GraphSAGE stack in `nn.GCN`'s shape: n_layers SAGEConv of one aggregator, `dropout(activation(norm(h)))` between them (BatchNorm1d
    with norm="batch": the fused epilogue), nothing after the last.  `forward` has `GCN.forward`'s contract, so the stack runs under
    train.train_step, minibatch.train_epoch, minibatch.subgraph_step and train_epoch_subgraphs unchanged."""

    def __init__(self, in_feats, n_classes, n_hidden, n_layers, activation, aggregator_type="mean", norm="none", dropout=0.0,
                 input_drop=0.0):
        super().__init__()
        if norm not in ("none", "batch"):
            raise ValueError(f'norm must be "none" or "batch", got {norm!r}')
        self.n_layers, self.n_hidden, self.n_classes = n_layers, n_hidden, n_classes
        self.convs, self.norms = nn.ModuleList(), nn.ModuleList()
        for i in range(n_layers):
            fin = n_hidden if i > 0 else in_feats
            fout = n_hidden if i < n_layers - 1 else n_classes
            last = i == n_layers - 1
            self.convs.append(SAGEConv(fin, fout, aggregator_type, bias=norm == "none" or last))
            if not last and norm == "batch":
                self.norms.append(nn.BatchNorm1d(fout))
        self.input_drop, self.dropout = nn.Dropout(input_drop), nn.Dropout(dropout)
        self.activation = activation

    def forward(self, graph, feat=None, edge_weight=None):
        """`graph`: a Graph (`feat` in original node order), or a list of n_layers sampled blocks: layer i runs on blocks[i], `feat`
        defaults to blocks[0].srcdata["feat"].  `edge_weight`: a tensor for a Graph / Subgraph, a list of n_layers tensors for a block
        list (one per block); each reaches its layer's `SAGEConv`."""
        blocks = _block_list(graph, feat, self.n_layers)
        if edge_weight is not None:
            if blocks is None:
                if isinstance(edge_weight, (list, tuple)):
                    raise ValueError("a stack called on a Graph takes one edge_weight tensor, not a list")
            elif not isinstance(edge_weight, (list, tuple)) or len(edge_weight) != self.n_layers:
                raise ValueError(f"a block list takes a list of {self.n_layers} edge_weight tensors, one per block")
        h = graph.to_internal(feat) if blocks is None else (blocks[0].srcdata["feat"] if feat is None else feat)
        h = self.input_drop(h)
        for i in range(self.n_layers):
            g = graph if blocks is None else blocks[i]
            if edge_weight is None:
                h = self.convs[i](g, h)
            else:
                h = self.convs[i](g, h, edge_weight=edge_weight if blocks is None else edge_weight[i])
            if i < self.n_layers - 1:
                if len(self.norms):
                    h = _epilogue(h, self.norms[i], self.activation, self.dropout, self.training)
                else:
                    h = self.dropout(self.activation(h))
        return h if blocks is not None else graph.to_original(h)
