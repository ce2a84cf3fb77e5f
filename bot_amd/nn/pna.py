"""Principal Neighbourhood Aggregation (Corso, Cavalleri, Beaini, Lio, Velickovic, NeurIPS 2020): `PNAConv`, interface-identical to
DGL 1.x's `dgl.nn.PNAConv` where DESIGN §1 states it, `pna_delta`, and the `PNA` stack in `nn.GCN`'s shape.

DGL's per-edge "pretrans" M(cat[h_u, h_v]) is linear, so the message on u -> v is a[u] + b[v] with a = h W_s^T and b = h_dst W_d^T + bias:
no [E, F] message tensor exists.  ONE `ops.linear` gives every tower's `a` (a block-diagonal arrangement of the towers' W_s), one the
`b`, and ONE sweep per layer (`ops.pna_aggregate`, csrc/spmm_pna.hip) aggregates all towers: every aggregator of the same gathered row,
the scalers and the tower-major layout in its epilogue.

With edge features (DGL's `PNAConv(edge_feat_size=K)`) the pretrans is M(cat[h_u, h_v, e_uv]), still linear: the message gains the term
W_e e_uv, which `ops.pna_aggregate_edge` (csrc/spmm_pna_edge.hip) forms inside the gather from the K raw floats of the edge.  That is
`EdgePNAConv` / `EdgePNA`, classes of their own: `PNAConv` keeps refusing edge features, as its tests pin.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops
from ..errors import DGLError
from . import _block_list, _sampled, _src_rows

__all__ = ["PNAConv", "PNA", "EdgePNAConv", "EdgePNA", "pna_delta"]


def pna_delta(graph) -> float:
    """The normalisation constant of the PNA scalers: the mean over the nodes of log(in_degree + 1).  One host read."""
    return float(torch.log(graph.in_degrees().to(torch.float32) + 1.0).mean())


class _Tower(nn.Module):
    """The parameters of one tower under DGL's names: M (the pretrans), U (the posttrans), batchnorm."""

    def __init__(self, in_size, out_size, n_blocks, edge_feat_size=0):
        super().__init__()
        self.M = nn.Linear(2 * in_size + edge_feat_size, in_size)
        self.U = nn.Linear((n_blocks + 1) * in_size, out_size)
        self.batchnorm = nn.BatchNorm1d(out_size)


class _PNAConvBase(nn.Module):
    """What `PNAConv` and `EdgePNAConv` share: the parameters under DGL's names and the forward around the one aggregation call."""

    def __init__(self, who, in_size, out_size, aggregators, scalers, delta, dropout, num_towers, edge_feat_size, residual):
        super().__init__()
        self.aggregators, self.scalers = ops.pna_check_names(aggregators, scalers)
        if num_towers < 1 or in_size % num_towers or out_size % num_towers:
            raise DGLError(f"{who}: num_towers = {num_towers} must divide in_size = {in_size} and out_size = {out_size}")
        self.in_size, self.out_size, self.num_towers, self.delta = in_size, out_size, num_towers, float(delta)
        self.tower_in_size, self.tower_out_size = in_size // num_towers, out_size // num_towers
        self.edge_feat_size = int(edge_feat_size)
        self.residual = bool(residual) and in_size == out_size
        n_blocks = len(self.aggregators) * len(self.scalers)
        self.towers = nn.ModuleList([_Tower(self.tower_in_size, self.tower_out_size, n_blocks, self.edge_feat_size)
                                     for _ in range(num_towers)])
        self.dropout = nn.Dropout(dropout)
        self.mixing_layer = nn.Sequential(nn.Linear(out_size, out_size), nn.LeakyReLU())

    def _run(self, who, graph, node_feat, edge_feat, impl):
        if graph.halo is not None:
            raise ValueError(f"{who} on a partitioned graph (a halo plan) is not supported: it takes whole graphs, Subgraphs and "
                             "sampled blocks")
        n_dst = graph.number_of_dst_nodes()
        if isinstance(node_feat, tuple):
            h_src, h_dst = _src_rows(graph, node_feat[0]), node_feat[1]
            if h_dst.shape[0] != n_dst:
                raise ValueError(f"feat_dst holds {h_dst.shape[0]} rows, the graph has {n_dst} destination nodes")
        else:
            h_src = _src_rows(graph, node_feat)
            h_dst = h_src[:n_dst] if _sampled(graph) else h_src
        Ft, T = self.tower_in_size, self.num_towers
        Ms = [t.M.weight for t in self.towers]
        w_src = Ms[0][:, :Ft].contiguous() if T == 1 else torch.block_diag(*[m[:, :Ft] for m in Ms])
        w_dst = Ms[0][:, Ft:2 * Ft].contiguous() if T == 1 else torch.block_diag(*[m[:, Ft:2 * Ft] for m in Ms])
        bias = self.towers[0].M.bias if T == 1 else torch.cat([t.M.bias for t in self.towers])
        a = ops.linear(h_src, w_src)                       # all towers' W_s h_u: one product
        b = ops.linear(h_dst, w_dst, bias)                 # all towers' W_d h_v + bias
        if edge_feat is None:
            agg = ops.pna_aggregate(graph, a, b, self.aggregators, self.scalers, self.delta, tower_width=Ft, impl=impl)   # ONE sweep
        else:                                              # every tower sees the whole edge feature: the towers' edge columns, stacked
            w_edge = Ms[0][:, 2 * Ft:].contiguous() if T == 1 else torch.cat([m[:, 2 * Ft:] for m in Ms])      # [F, K]
            agg = ops.pna_aggregate_edge(graph, a, b, edge_feat, w_edge, self.aggregators, self.scalers, self.delta, tower_width=Ft,
                                         impl=impl)                                                               # ONE sweep
        W = agg.shape[1] // T                              # a tower's S*A*Ft columns: a contiguous range of the row
        snorm = 1.0 / math.sqrt(max(n_dst, 1))
        outs = []
        for t, tower in enumerate(self.towers):
            h_t, agg_t = h_dst[:, t * Ft:(t + 1) * Ft], agg[:, t * W:(t + 1) * W]
            if T > 1:                                      # ops.linear takes whole rows: a tower's slice is copied
                h_t, agg_t = h_t.contiguous(), agg_t.contiguous()
            u_h, u_agg = tower.U.weight[:, :Ft].contiguous(), tower.U.weight[:, Ft:].contiguous()
            z = ops.linear(h_t, u_h) + ops.linear(agg_t, u_agg, tower.U.bias)      # U_h h_t + U_agg agg_t: no cat of [h, agg]
            outs.append(self.dropout(tower.batchnorm(z * snorm)))
        h = outs[0] if T == 1 else torch.cat(outs, dim=1)
        lin = self.mixing_layer[0]
        h = self.mixing_layer[1](ops.linear(h, lin.weight, lin.bias))
        return h + h_dst if self.residual else h

    def extra_repr(self):
        edge = f", edge_feat_size={self.edge_feat_size}" if self.edge_feat_size else ""
        return (f"in={self.in_size}, out={self.out_size}, towers={self.num_towers}{edge}, aggregators={self.aggregators}, "
                f"scalers={self.scalers}, delta={self.delta:.4g}")


class PNAConv(_PNAConvBase):
    """PNA layer (DGL 1.x `PNAConv`).  Per tower t on the column slice h_t of the input:

        message   M([h_u, h_v]) on every edge u -> v
        h_neigh   every aggregator of the messages times every scaler of the in-degree (`ops.pna_aggregate`)
        z         U(cat[h_t, h_neigh]) / sqrt(n_dst), then dropout(batchnorm(z))

    the towers' outputs side by side, then LeakyReLU(0.01)(Linear(out, out)), + the input when `residual` and in_size == out_size.
    `graph`: a whole Graph, a Subgraph or a sampled Block (destinations = the first n_dst source rows); `feat`: a tensor or a
    (feat_src, feat_dst) pair.  A partition with a halo plan raises ValueError; edge features are `EdgePNAConv`'s (here:
    NotImplementedError)."""

    def __init__(self, in_size, out_size, aggregators, scalers, delta, dropout=0.0, num_towers=1, edge_feat_size=0, residual=True):
        if edge_feat_size > 0:
            raise NotImplementedError("PNAConv: edge features (edge_feat_size > 0) are EdgePNAConv's (DESIGN §1); PNAConv takes none")
        super().__init__("PNAConv", in_size, out_size, aggregators, scalers, delta, dropout, num_towers, 0, residual)

    def forward(self, graph, node_feat, edge_feat=None, impl=None):
        if edge_feat is not None:
            raise NotImplementedError("PNAConv: edge features are EdgePNAConv's (DESIGN §1); this layer was built without them")
        return self._run("PNAConv", graph, node_feat, None, impl)


class EdgePNAConv(_PNAConvBase):
    """`PNAConv` with DGL's `edge_feat_size=K`: the message of tower t on u -> v is M_t(cat[h_u, h_v, e_uv]) with e_uv the K raw
    features of the edge - every tower sees the whole edge feature - so `towers.{t}.M.weight` is [Ft, 2 Ft + K], columns
    [h_u | h_v | e]; everything else is `PNAConv`'s.  The towers' edge columns, stacked to [F, K], are the one weight of the one sweep
    per layer (`ops.pna_aggregate_edge`): no [E, F] message exists in the kernel form.  `edge_feat`: [E, K] in edge-id order (on a Block
    or Subgraph that is the CSC position).  A halo plan, a missing or a mis-shaped `edge_feat` raise ValueError."""

    def __init__(self, in_size, out_size, aggregators, scalers, delta, dropout=0.0, num_towers=1, edge_feat_size=1, residual=True):
        if int(edge_feat_size) < 1:
            raise ValueError(f"EdgePNAConv: edge_feat_size must be at least 1, got {edge_feat_size} (PNAConv is the layer without edge features)")
        super().__init__("EdgePNAConv", in_size, out_size, aggregators, scalers, delta, dropout, num_towers, edge_feat_size, residual)

    def forward(self, graph, node_feat, edge_feat, impl=None):
        E, K = graph.number_of_edges(), self.edge_feat_size
        if edge_feat is None or edge_feat.dim() != 2 or tuple(edge_feat.shape) != (E, K):
            raise ValueError(f"EdgePNAConv: edge_feat must be [{E}, {K}] (one row per edge, edge-id order), got "
                             f"{None if edge_feat is None else tuple(edge_feat.shape)}")
        return self._run("EdgePNAConv", graph, node_feat, edge_feat, impl)


class PNA(nn.Module):
    """PNA stack in `nn.GCN`'s shape: encoder Linear(in_feats, n_hidden), n_layers PNAConv(n_hidden, n_hidden) with residual and
    `dropout(relu(h))` between them, decoder Linear(n_hidden, n_classes).  `forward` has `GCN.forward`'s contract, so the stack runs
    under train.train_step, minibatch.train_epoch, minibatch.subgraph_step and train_epoch_subgraphs unchanged."""

    def __init__(self, in_feats, n_classes, n_hidden, n_layers, aggregators=("mean", "max", "min", "std"),
                 scalers=("identity", "amplification", "attenuation"), delta=1.0, num_towers=1, dropout=0.0, input_drop=0.0):
        super().__init__()
        self.n_layers, self.n_hidden, self.n_classes = n_layers, n_hidden, n_classes
        self.encoder = nn.Linear(in_feats, n_hidden)
        self.convs = nn.ModuleList([PNAConv(n_hidden, n_hidden, aggregators, scalers, delta, num_towers=num_towers, residual=True)
                                    for _ in range(n_layers)])
        self.decoder = nn.Linear(n_hidden, n_classes)
        self.input_drop, self.dropout = nn.Dropout(input_drop), nn.Dropout(dropout)

    def forward(self, graph, feat=None):
        """`graph`: a Graph (`feat` in original node order), or a list of n_layers sampled blocks: layer i runs on blocks[i], `feat`
        defaults to blocks[0].srcdata["feat"]."""
        blocks = _block_list(graph, feat, self.n_layers)
        h = graph.to_internal(feat) if blocks is None else (blocks[0].srcdata["feat"] if feat is None else feat)
        h = ops.linear(self.input_drop(h), self.encoder.weight, self.encoder.bias)
        for i in range(self.n_layers):
            h = self.convs[i](graph if blocks is None else blocks[i], h)
            if i < self.n_layers - 1:
                h = self.dropout(F.relu(h))
        h = ops.linear(h, self.decoder.weight, self.decoder.bias)
        return h if blocks is not None else graph.to_original(h)


class EdgePNA(nn.Module):
    """The `PNA` stack over `EdgePNAConv(edge_feat_size=edge_dim)` layers.  `forward(graph, feat=None, edge_feats=None)` hands each layer
    the raw edge features of its graph (`nn.gen.layer_edge_feats`): a tensor, an `edata` key, edata["feat"] by default, or a list of one
    tensor per block."""

    def __init__(self, in_feats, n_classes, n_hidden, n_layers, edge_dim, aggregators=("mean", "max", "min", "std"),
                 scalers=("identity", "amplification", "attenuation"), delta=1.0, num_towers=1, dropout=0.0, input_drop=0.0):
        super().__init__()
        self.n_layers, self.n_hidden, self.n_classes, self.edge_dim = n_layers, n_hidden, n_classes, int(edge_dim)
        self.encoder = nn.Linear(in_feats, n_hidden)
        self.convs = nn.ModuleList([EdgePNAConv(n_hidden, n_hidden, aggregators, scalers, delta, num_towers=num_towers,
                                                edge_feat_size=edge_dim, residual=True) for _ in range(n_layers)])
        self.decoder = nn.Linear(n_hidden, n_classes)
        self.input_drop, self.dropout = nn.Dropout(input_drop), nn.Dropout(dropout)

    def forward(self, graph, feat=None, edge_feats=None):
        from .gen import layer_edge_feats
        blocks = _block_list(graph, feat, self.n_layers)
        efs = layer_edge_feats("EdgePNA", self.edge_dim, self.n_layers, graph, blocks, edge_feats)
        h = graph.to_internal(feat) if blocks is None else (blocks[0].srcdata["feat"] if feat is None else feat)
        h = ops.linear(self.input_drop(h), self.encoder.weight, self.encoder.bias)
        for i in range(self.n_layers):
            h = self.convs[i](graph if blocks is None else blocks[i], h, efs[i])
            if i < self.n_layers - 1:
                h = self.dropout(F.relu(h))
        h = ops.linear(h, self.decoder.weight, self.decoder.bias)
        return h if blocks is not None else graph.to_original(h)
