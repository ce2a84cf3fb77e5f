"""APPNP (Gasteiger, Bojchevski, Günnemann, "Predict then Propagate", ICLR 2019): `APPNPConv`, DGL's, and the paper's `APPNP` model;
GCNII (Chen, Wei, Huang, Ding, Li, "Simple and Deep Graph Convolutional Networks", ICML 2020): `GCN2Conv`, DGL's, and a `GCNII` stack.

Both are (1 - alpha) P h + alpha h0, repeated, on `ops.appnp_propagate` (bot_amd/appnp.py, csrc/appnp.hip): one launch per step and
direction, the per-step edge dropout regenerated from a seed, nothing of size [N, C] saved for the backward.  GCN2Conv's identity mapping
(1 - beta) r + beta r W is ONE product with the [F, F] operand (1 - beta) I + beta W, not an axpy pass over [N, F].
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from .. import gemm, ops
from ..appnp import propagate_scaled
from . import _block_list, _epilogue

__all__ = ["APPNPConv", "APPNP", "GCN2Conv", "GCNII"]


def _graph_only(graph, feat, who):
    if isinstance(graph, (list, tuple)):
        raise ValueError(f"{who} takes a whole Graph or a Subgraph, not a block list: the propagation needs a square graph (DESIGN §8)")
    _block_list(graph, feat, 0)


class APPNPConv(nn.Module):
    """DGL's `APPNPConv(k, alpha, edge_drop)`: h_0 = feat, h_t = (1 - alpha) P_t h_{t-1} + alpha feat for t = 1..k with
    P_t = D^-1/2 (A o M_t) D^-1/2, D the in-degree clamped at 1 (with `edge_weight`, float32 [E] / [E, 1] in edge-id order and constant:
    the weighted in-degree).  No parameters.  `edge_drop` is active only in training mode; each call draws one seed and step t uses
    counter word t."""

    def __init__(self, k, alpha, edge_drop=0.0):
        super().__init__()
        self._k, self._alpha, self.edge_drop = int(k), float(alpha), float(edge_drop)

    def forward(self, graph, feat, edge_weight=None):
        shape = feat.shape
        h = ops.appnp_propagate(graph, feat.reshape(shape[0], -1), self._k, self._alpha, edge_drop=self.edge_drop if self.training else 0.0,
                                edge_weight=edge_weight)
        return h.view(shape)

    def extra_repr(self):
        return f"k={self._k}, alpha={self._alpha}, edge_drop={self.edge_drop}"


class APPNP(nn.Module):
    """The paper's model: an MLP of `n_layers` linear layers (`lins`), `dropout(activation(norm(h)))` between them (BatchNorm1d `norms`
    with norm="batch": the fused epilogue), then one `APPNPConv` (`propagate`) on the logits.  `forward` has `nn.GCN`'s contract for a
    Graph / Subgraph (`feat` in original node order); a block list raises ValueError."""

    def __init__(self, in_feats, n_classes, n_hidden, n_layers, activation, k=10, alpha=0.1, edge_drop=0.5, dropout=0.5, input_drop=0.0,
                 norm="none"):
        super().__init__()
        if norm not in ("none", "batch"):
            raise ValueError(f'norm must be "none" or "batch", got {norm!r}')
        self.n_layers, self.n_hidden, self.n_classes = n_layers, n_hidden, n_classes
        self.lins, self.norms = nn.ModuleList(), nn.ModuleList()
        for i in range(n_layers):
            last = i == n_layers - 1
            self.lins.append(nn.Linear(n_hidden if i > 0 else in_feats, n_classes if last else n_hidden, bias=norm == "none" or last))
            if not last and norm == "batch":
                self.norms.append(nn.BatchNorm1d(n_hidden))
        self.propagate = APPNPConv(k, alpha, edge_drop)
        self.input_drop, self.dropout = nn.Dropout(input_drop), nn.Dropout(dropout)
        self.activation = activation

    def forward(self, graph, feat=None, edge_weight=None):
        _graph_only(graph, feat, "APPNP")
        h = self.input_drop(graph.to_internal(feat))
        for i, lin in enumerate(self.lins):
            h = ops.linear(h, lin.weight, lin.bias)
            if i < self.n_layers - 1:
                if len(self.norms):
                    h = _epilogue(h, self.norms[i], self.activation, self.dropout, self.training)
                else:
                    h = self.dropout(self.activation(h))
        return graph.to_original(self.propagate(graph, h, edge_weight=edge_weight))


class GCN2Conv(nn.Module):
    """DGL's `GCN2Conv`.  With beta = log(lambda_ / layer + 1) and s = (1 - alpha) P feat, P = D^-1/2 A D^-1/2 (in-degree clamped at 1):
        project_initial_features=True    r = s + alpha feat_0;  (1 - beta) r + beta r weight1
        project_initial_features=False   (1 - beta) (s + alpha feat_0) + beta (s weight1 + alpha feat_0 weight2)
    then + bias, then `activation`.  No edge dropout (DGL's has none).  Gradients reach feat, feat_0 and the parameters."""

    def __init__(self, in_feats, layer, alpha=0.1, lambda_=1, project_initial_features=True, bias=True, activation=None):
        super().__init__()
        self._in_feats, self._project_initial_features, self._activation = in_feats, project_initial_features, activation
        self.alpha, self.beta = float(alpha), math.log(lambda_ / layer + 1)
        self.weight1 = nn.Parameter(torch.empty(in_feats, in_feats))
        if project_initial_features:
            self.register_parameter("weight2", None)
        else:
            self.weight2 = nn.Parameter(torch.empty(in_feats, in_feats))
        if bias:
            self.bias = nn.Parameter(torch.empty(in_feats))
        else:
            self.register_parameter("bias", None)
        self.reset_parameters()

    def reset_parameters(self):
        nn.init.normal_(self.weight1)
        if self.weight2 is not None:
            nn.init.normal_(self.weight2)
        if self.bias is not None:
            nn.init.zeros_(self.bias)

    def _mapping(self, w):
        """(1 - beta) I + beta w: the [F, F] operand of the identity mapping."""
        eye = torch.eye(self._in_feats, dtype=w.dtype, device=w.device)
        return (1.0 - self.beta) * eye + self.beta * w

    def forward(self, graph, feat, feat_0, edge_weight=None):
        if self._project_initial_features:
            r = ops.appnp_propagate(graph, feat, 1, self.alpha, h0=feat_0, edge_weight=edge_weight)
            rst = gemm.matmul(r, self._mapping(self.weight1))
        else:
            s = propagate_scaled(graph, feat, 1.0 - self.alpha, edge_weight=edge_weight)
            rst = gemm.matmul(s, self._mapping(self.weight1)) + gemm.matmul(self.alpha * feat_0, self._mapping(self.weight2))
        if self.bias is not None:   # the bias gradient, a column sum over N rows, comes from the library's kernel on the GPU
            rst = ops.add_bias(rst, self.bias) if rst.is_cuda else rst + self.bias
        return rst if self._activation is None else self._activation(rst)

    def extra_repr(self):
        return f"in={self._in_feats}, alpha={self.alpha}, beta={self.beta:.4f}, project_initial_features={self._project_initial_features}"


class GCNII(nn.Module):
    """GCNII: a linear layer (`lins.0`), n_layers x (dropout, `GCN2Conv(layer=i + 1)`, activation) (`convs`), dropout, a linear layer
    (`lins.1`); feat_0 is the first linear's activated output.  `forward` has `APPNP.forward`'s contract."""

    def __init__(self, in_feats, n_classes, n_hidden, n_layers, activation, alpha=0.1, lambda_=0.5, dropout=0.5, input_drop=0.0):
        super().__init__()
        self.n_layers, self.n_hidden, self.n_classes = n_layers, n_hidden, n_classes
        self.lins = nn.ModuleList([nn.Linear(in_feats, n_hidden), nn.Linear(n_hidden, n_classes)])
        self.convs = nn.ModuleList([GCN2Conv(n_hidden, i + 1, alpha, lambda_) for i in range(n_layers)])
        self.input_drop, self.dropout = nn.Dropout(input_drop), nn.Dropout(dropout)
        self.activation = activation

    def reset_parameters(self):
        for m in list(self.lins) + list(self.convs):
            m.reset_parameters()

    def forward(self, graph, feat=None, edge_weight=None):
        _graph_only(graph, feat, "GCNII")
        h = self.input_drop(graph.to_internal(feat))
        h = h0 = self.activation(ops.linear(h, self.lins[0].weight, self.lins[0].bias))
        for conv in self.convs:
            h = self.activation(conv(graph, self.dropout(h), h0, edge_weight=edge_weight))
        h = self.dropout(h)
        return graph.to_original(ops.linear(h, self.lins[1].weight, self.lins[1].bias))
