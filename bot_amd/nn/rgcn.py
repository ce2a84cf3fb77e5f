"""Relational graph convolution (Schlichtkrull et al., "Modeling Relational Data with Graph Convolutional Networks", ESWC 2018):
`RelGraphConv` with the surface of DGL 0.6's layer of that name where DESIGN §1 states it, the entity-classification norm `rel_norm`,
and the `RGCN` stack in `nn.GCN`'s shape.

One node set, typed edges: out[v] = sum_r sum_{u in N_r(v)} c_e W_r h_u with the basis regulariser W_r = sum_b w_comp[r, b] V_b.  The
relation part is ONE dense GEMM and ONE sweep of `ops.rel_expand_sum` / `ops.rel_contract_sum` (csrc/spmm_rel.hip): the relation rides
beside the source id, the per-relation weights never meet the edges, and nothing of size [E, F] or [E, B, F] exists in either pass.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import gemm, ops
from ..errors import DGLError
from . import _block_list, _epilogue, _sampled, _src_rows

__all__ = ["RelGraphConv", "RGCN", "rel_norm"]


def rel_norm(g, etypes, num_rels):
    """The entity-classification norm: float32 [E, 1] (edge-id order) whose entry e = (u -> v) is 1 / (the number of in-edges of v with
    e's relation).  Integer counting in tensor ops, once per graph and relation tensor.  etypes: int32 / int64 [E] or an edata key."""
    if isinstance(etypes, str):
        etypes = g.edata[etypes]
    E = g.number_of_edges()
    if etypes.dtype not in (torch.int32, torch.int64) or tuple(etypes.shape) != (E,):
        raise DGLError(f"rel_norm: etypes must be an int32 or int64 tensor [{E}], got {tuple(etypes.shape)} {etypes.dtype}")

    def make():
        key = g.edges()[1].to(etypes.device) * num_rels + etypes.long()
        if E and (int(etypes.min()) < 0 or int(etypes.max()) >= num_rels):
            raise DGLError(f"rel_norm: etypes must lie in [0, num_rels = {num_rels})")
        count = torch.bincount(key, minlength=g.number_of_dst_nodes() * num_rels)
        return (1.0 / count[key].to(torch.float32)).reshape(E, 1)
    return ops._rel_cached(g, etypes, ("rel_norm", num_rels), make)


class RelGraphConv(nn.Module):
    """`dgl.nn.RelGraphConv` (DGL 0.6) on one fused relation sweep:

        out = dropout(activation(layer_norm(sum_e c_e W_{r_e} h_u + h_bias + h_v @ loop_weight)))

    Parameters: `weight` [num_bases, in_feat, out_feat]; `w_comp` [num_rels, num_bases] with regularizer="basis" and num_bases <
    num_rels (absent otherwise: one weight per relation, the sweeps' one-hot mode); `h_bias`; `loop_weight`; `layer_norm_weight` (a
    `torch.nn.LayerNorm` with affine parameters).  `low_mem` is accepted and ignored; regularizer="bdd" raises NotImplementedError.

    The GEMM order follows GraphConv's rule: in_feat <= out_feat aggregates first (`ops.rel_expand_sum`, then one [n, B in] x [B in, out]
    product), else projects first (one [n, in] x [in, B out] product, then `ops.rel_contract_sum`); the `order` attribute ("aggregate" |
    "project" | None) overrides it.  `forward(g, feat, etypes, norm=None)`: a whole Graph, a Subgraph or a sampled Block (destinations =
    the first n_dst sources); feat a tensor or a (feat_src, feat_dst) pair; etypes / norm tensors in edge-id order or edata keys."""

    def __init__(self, in_feat, out_feat, num_rels, regularizer="basis", num_bases=None, bias=True, activation=None, self_loop=True,
                 low_mem=False, dropout=0.0, layer_norm=False):
        super().__init__()
        if regularizer == "bdd":
            raise NotImplementedError('RelGraphConv: regularizer="bdd" (block-diagonal decomposition) is not implemented; use "basis" or None')
        if regularizer not in ("basis", None):
            raise ValueError(f'regularizer must be "basis", "bdd" or None, got {regularizer!r}')
        if num_rels < 1:
            raise ValueError(f"num_rels must be at least 1, got {num_rels}")
        if regularizer is None or num_bases is None or num_bases > num_rels or num_bases <= 0:
            num_bases = num_rels
        self.in_feat, self.out_feat, self.num_rels, self.regularizer, self.num_bases = in_feat, out_feat, num_rels, regularizer, num_bases
        self.bias, self.activation, self.self_loop, self.low_mem, self.layer_norm = bias, activation, self_loop, low_mem, layer_norm
        self.order = None
        self.weight = nn.Parameter(torch.empty(num_bases, in_feat, out_feat))
        if num_bases < num_rels:
            self.w_comp = nn.Parameter(torch.empty(num_rels, num_bases))
        else:
            self.register_parameter("w_comp", None)
        if bias:
            self.h_bias = nn.Parameter(torch.empty(out_feat))
        else:
            self.register_parameter("h_bias", None)
        if layer_norm:
            self.layer_norm_weight = nn.LayerNorm(out_feat, elementwise_affine=True)
        if self_loop:
            self.loop_weight = nn.Parameter(torch.empty(in_feat, out_feat))
        else:
            self.register_parameter("loop_weight", None)
        self.dropout = nn.Dropout(dropout)
        self.reset_parameters()

    def reset_parameters(self):
        gain = nn.init.calculate_gain("relu")
        nn.init.xavier_uniform_(self.weight, gain=gain)
        if self.w_comp is not None:
            nn.init.xavier_uniform_(self.w_comp)
        if self.h_bias is not None:
            nn.init.zeros_(self.h_bias)
        if self.loop_weight is not None:
            nn.init.xavier_uniform_(self.loop_weight, gain=gain)

    def aggregate_first(self):
        if self.order not in (None, "aggregate", "project"):
            raise ValueError(f'order must be "aggregate", "project" or None, got {self.order!r}')
        return self.in_feat <= self.out_feat if self.order is None else self.order == "aggregate"

    def forward(self, g, feat, etypes, norm=None):
        if g.halo is not None:
            raise ValueError("RelGraphConv on a partitioned graph (a halo plan) is not supported: it takes whole graphs, Subgraphs and "
                             "sampled blocks")
        n_dst = g.number_of_dst_nodes()
        if isinstance(feat, tuple):
            h_src, h_dst = _src_rows(g, feat[0]), feat[1]
            if h_dst.shape[0] != n_dst:
                raise ValueError(f"feat_dst holds {h_dst.shape[0]} rows, the graph has {n_dst} destination nodes")
        else:
            h_src = _src_rows(g, feat)
            h_dst = h_src[:n_dst] if _sampled(g) else h_src      # a block's destinations are its first n_dst sources
        if h_src.dim() != 2 or h_src.shape[1] != self.in_feat:
            raise DGLError(f"RelGraphConv takes features [n_src, in_feat = {self.in_feat}], got {tuple(h_src.shape)}")
        B, Fi, Fo = self.num_bases, self.in_feat, self.out_feat
        if self.aggregate_first():
            z = ops.rel_expand_sum(g, h_src, etypes, self.num_rels, self.w_comp, norm)                 # [n_dst, B, in]
            rst = gemm.matmul(z.reshape(n_dst, B * Fi), self.weight.reshape(B * Fi, Fo))
        else:
            y = gemm.matmul(h_src, self.weight.permute(1, 0, 2).reshape(Fi, B * Fo))                    # x @ [V_1 | ... | V_B]
            rst = ops.rel_contract_sum(g, y.view(-1, B, Fo), etypes, self.num_rels, self.w_comp, norm)
        if self.loop_weight is not None:
            rst = torch.addmm(rst, h_dst, self.loop_weight)
        if self.h_bias is not None:
            rst = ops.add_bias(rst, self.h_bias) if rst.is_cuda and rst.dtype == torch.float32 else rst + self.h_bias
        if self.layer_norm:
            rst = self.layer_norm_weight(rst)
        if self.activation is not None:
            rst = self.activation(rst)
        return self.dropout(rst)

    def extra_repr(self):
        return (f"in={self.in_feat}, out={self.out_feat}, num_rels={self.num_rels}, regularizer={self.regularizer!r}, "
                f"num_bases={self.num_bases}, self_loop={self.self_loop}")


class RGCN(nn.Module):
    """R-GCN stack in `nn.GCN`'s shape: n_layers RelGraphConv, `dropout(activation(norm(h)))` between them (BatchNorm1d with
    norm="batch": the fused epilogue), nothing after the last.  `etypes` / `norm` default to the graph's (each block's) edata["etype"] /
    edata["norm"] when present - the frames of a Block or a Subgraph gather them from the parent - so the stack runs under
    train.train_step, minibatch.train_epoch and train_epoch_subgraphs unchanged."""

    def __init__(self, in_feats, n_classes, n_hidden, n_layers, num_rels, activation, regularizer="basis", num_bases=None, norm="none",
                 dropout=0.0, input_drop=0.0, self_loop=True):
        super().__init__()
        if norm not in ("none", "batch"):
            raise ValueError(f'norm must be "none" or "batch", got {norm!r}')
        self.n_layers, self.n_hidden, self.n_classes, self.num_rels = n_layers, n_hidden, n_classes, num_rels
        self.convs, self.norms = nn.ModuleList(), nn.ModuleList()
        for i in range(n_layers):
            last = i == n_layers - 1
            fout = n_classes if last else n_hidden
            self.convs.append(RelGraphConv(n_hidden if i > 0 else in_feats, fout, num_rels, regularizer=regularizer, num_bases=num_bases,
                                           bias=norm == "none" or last, self_loop=self_loop))
            if not last and norm == "batch":
                self.norms.append(nn.BatchNorm1d(fout))
        self.input_drop, self.dropout = nn.Dropout(input_drop), nn.Dropout(dropout)
        self.activation = activation

    @staticmethod
    def _edge_input(g, given, key, required):
        if given is not None:
            return given
        if key in g.edata:
            return key
        if required:
            raise DGLError(f"RGCN: pass etypes or store them as edata[{key!r}]")
        return None

    def forward(self, graph, feat=None, etypes=None, norm=None):
        """`graph`: a Graph (`feat` in original node order), or a list of n_layers sampled blocks: layer i runs on blocks[i], `feat`
        defaults to blocks[0].srcdata["feat"].  etypes / norm: a tensor or an edata key (a list of n_layers of them for a block list)."""
        blocks = _block_list(graph, feat, self.n_layers)
        for name, v in (("etypes", etypes), ("norm", norm)):
            if blocks is not None and v is not None and not isinstance(v, str) and (not isinstance(v, (list, tuple)) or len(v) != self.n_layers):
                raise ValueError(f"a block list takes {name} as an edata key or a list of {self.n_layers}, one per block")
        h = graph.to_internal(feat) if blocks is None else (blocks[0].srcdata["feat"] if feat is None else feat)
        h = self.input_drop(h)
        for i in range(self.n_layers):
            g = graph if blocks is None else blocks[i]
            pick = lambda v: v[i] if isinstance(v, (list, tuple)) else v
            h = self.convs[i](g, h, self._edge_input(g, pick(etypes), "etype", True), self._edge_input(g, pick(norm), "norm", False))
            if i < self.n_layers - 1:
                if len(self.norms):
                    h = _epilogue(h, self.norms[i], self.activation, self.dropout, self.training)
                else:
                    h = self.dropout(self.activation(h))
        return h if blocks is not None else graph.to_original(h)
