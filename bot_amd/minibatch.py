"""Mini-batch training and evaluation over sampled blocks — the loops of src/ogbn-products/gat.py:113-193 and
src/ogbn-proteins/gat.py:96-171, on `bot_amd.sampling.NodeDataLoader` batches — and training over induced-subgraph (cluster)
batches, `bot_amd.sampling.ClusterLoader`: the full-batch step of `bot_amd.train`, run on one `Subgraph` at a time."""
from __future__ import annotations

import torch

__all__ = ["add_labels", "train_epoch", "evaluate", "evaluate_scores", "node_roles", "subgraph_step", "train_epoch_subgraphs"]


def add_labels(block, idx, n_classes):
    """ogbn-products/gat.py:105-110: the block's source features get `n_classes` more columns, the parent's
    `train_labels_onehot` rows at the source positions `idx` and zeros elsewhere."""
    feat = block.srcdata["feat"]
    onehot = torch.zeros((feat.shape[0], n_classes), dtype=feat.dtype, device=feat.device)
    onehot[idx] = block.srcdata["train_labels_onehot"][idx].to(feat.dtype)
    block.srcdata["feat"] = torch.cat([feat, onehot], dim=-1)


def train_epoch(model, loader, labels, optimizer, loss, use_labels=False, n_classes=None):
    """One pass over `loader`: per batch the model runs on the blocks, `loss(pred, labels[output_nodes])` (a mean) is taken on
    the output nodes and the optimizer steps once.  With `use_labels` the labels of the input nodes beyond the outputs enter as
    features (add_labels).  Returns the output-count-weighted mean loss of the epoch (one host read per batch, as the reference's
    `loss.item()`)."""
    model.train()
    loss_sum, total = 0.0, 0
    for input_nodes, output_nodes, blocks in loader:
        n_out = int(output_nodes.numel())
        if use_labels:
            add_labels(blocks[0], torch.arange(n_out, int(input_nodes.numel()), device=input_nodes.device), n_classes)
        pred = model(blocks)
        value = loss(pred, labels[output_nodes])
        optimizer.zero_grad()
        value.backward()
        optimizer.step()
        loss_sum += float(value.detach()) * n_out
        total += n_out
    return loss_sum / max(total, 1)


@torch.no_grad()
def evaluate(model, loader, n_nodes, out_dim, eval_times=1, use_labels=False, n_classes=None):
    """Predictions [n_nodes, out_dim] averaged over `eval_times` passes of `loader` (fresh samples each pass); rows of nodes the
    loader never outputs stay zero.  With `use_labels` every input node's training label enters as a feature (gat.py:170-171)."""
    model.eval()
    dev = loader.g.device
    preds = torch.zeros((n_nodes, out_dim), dtype=torch.float32, device=dev)
    for _ in range(eval_times):
        for input_nodes, output_nodes, blocks in loader:
            if use_labels:
                add_labels(blocks[0], torch.arange(int(input_nodes.numel()), device=input_nodes.device), n_classes)
            preds[output_nodes] += model(blocks)
    return preds / eval_times


def node_roles(n_nodes, train_idx, val_idx=None, test_idx=None):
    """int8 [n_nodes] (original node order): 1 = training, 2 = validation, 3 = test node, 0 = none of them."""
    roles = torch.zeros(n_nodes, dtype=torch.int8, device=train_idx.device)
    for code, idx in ((1, train_idx), (2, val_idx), (3, test_idx)):
        if idx is not None:
            roles[idx] = code
    return roles


@torch.no_grad()
def evaluate_scores(model, loader, labels, train_idx, val_idx, test_idx, criterion, evaluator, eval_times=1, use_labels=False, n_classes=None):
    """The evaluation of ogbn-proteins/gat.py:135-171 and ogbn-products/gat.py:160-193: the predictions of `evaluate` over `loader`
    (all nodes it outputs, averaged over `eval_times` passes), then the reference's 7-tuple (train_score, val_score, test_score,
    train_loss, val_loss, test_loss, preds) with loss = `criterion(preds[idx], labels[idx])` read to the host per split.
    `evaluator`: a `bot_amd.metrics.Evaluator` - the three scores come from ONE grouped call over all rows, the groups being
    `node_roles` (one sort and one host read for "rocauc", not three); any other callable(pred, labels) -> score is applied per
    split, as the reference applies its `evaluator_wrapper`."""
    from .metrics import Evaluator
    n = labels.shape[0]
    out_dim = labels.shape[1] if n_classes is None else int(n_classes)
    preds = evaluate(model, loader, n, out_dim, eval_times=eval_times, use_labels=use_labels, n_classes=n_classes)
    splits = (train_idx, val_idx, test_idx)
    losses = [float(criterion(preds[idx], labels[idx])) for idx in splits]
    if isinstance(evaluator, Evaluator):
        groups = node_roles(n, train_idx.to(preds.device), val_idx.to(preds.device), test_idx.to(preds.device)) - 1
        scores = evaluator.eval_groups(preds, labels, groups, 3)
    else:
        scores = [evaluator(preds[idx], labels[idx]) for idx in splits]
    return (*scores, *losses, preds)


def subgraph_step(model, sub, optimizer, labels, roles, *, node_loss=None, step_kw=None, node_mask=None, loss_weight=None, edge_weight=None):
    """One train step on the `Subgraph` `sub`: what `workloads.build(name)` runs per step on the whole graph, on the batch.
    GCN / GAT stacks (`step_kw` given): `train.train_step` on (sub, sub.ndata["feat"], the batch's labels) with the training nodes
    inside the batch as local ids, so --labels, the mask rate and label reuse behave as in the full-batch step (`step_kw`: its
    keywords; validation / test nodes are located only when label reuse needs them).  Edge-feature stacks (`node_loss` given):
    `model(sub)`, which reads the gathered sub.ndata / sub.edata, and the mean of `node_loss` over the batch's training nodes.
    `labels` / `roles` (node_roles) / `node_mask` (bool [N]: the mask split of the step, per node, for tests) are in the parent's
    original node order, and so is `loss_weight` (float32 [N], `sampling.saint_loss_weights`): the batch's slice weights the loss
    as a self-normalised mean over the batch's prediction nodes (`train.forward_backward`; the edge-feature stacks: the per-node
    loss averaged over its trailing dimensions, sum lw y / sum lw), which for lw = 1 is the plain mean.  `edge_weight`: an `edata` key of the
    parent (GraphSAINT's aggregator normalisation, `sampling.saint_norms`): the batch's rows, `sub.edata[key]`, reach the GCN stack's
    layers as their `edge_weight`; a GAT stack (it learns its weights) or an edge-feature stack with one raises ValueError.  Returns (loss, pred, number of training nodes), or None when the batch holds no training node
    (nothing runs).  One device->host read (the training nodes' local ids)."""
    from . import train as T
    if edge_weight is not None:
        from . import nn as bnn
        if not isinstance(edge_weight, str):
            raise ValueError("edge_weight is an edata key of the parent graph")
        if step_kw is None or not isinstance(model, bnn.GCN):
            raise ValueError("edge_weight is for the GCN stacks: a GAT stack learns its edge weights, an edge-feature stack has none")
    rows = sub.parent_rows
    r = roles[rows]
    tr = torch.nonzero(r == 1).squeeze(1)
    if tr.numel() == 0:
        return None
    y = labels[rows]
    if step_kw is not None:
        kw = dict(step_kw)
        va = te = None
        if kw.get("n_label_iters", 0) > 0:
            va, te = torch.nonzero(r == 2).squeeze(1), torch.nonzero(r == 3).squeeze(1)
        if node_mask is not None:
            kw["mask"] = node_mask[rows][tr]
        if loss_weight is not None:
            kw["loss_weight"] = loss_weight[rows]
        if edge_weight is not None:
            kw["edge_weight"] = sub.edata[edge_weight]
        loss, pred = T.train_step(model, sub, sub.ndata["feat"], y, tr, va, te, optimizer, **kw)
    else:
        model.train()
        optimizer.zero_grad()
        pred = model(sub)
        if loss_weight is None:
            loss = node_loss(pred[tr], y[tr]).mean()
        else:
            per_node = node_loss(pred[tr], y[tr])
            per_node = per_node.reshape(per_node.shape[0], -1).mean(1)
            w = loss_weight[rows][tr].to(per_node.dtype)
            loss = (w * per_node).sum() / w.sum()
        loss.backward()
        optimizer.step()
    return loss, pred, int(tr.numel())


def train_epoch_subgraphs(model, loader, optimizer, labels, train_idx, *, val_idx=None, test_idx=None, node_loss=None, step_kw=None,
                          node_mask=None, loss_weight=None, edge_weight=None):
    """One pass over a `ClusterLoader` or `SAINTLoader`: `subgraph_step` per batch (a batch without training nodes is skipped and
    counted); `loss_weight` ([N], the parent's original order) and `edge_weight` (an edata key of the parent) as there.
    Returns (mean loss of the epoch weighted by the batches' training-node counts, number of skipped batches); one host read of
    the loss per batch, as `train_epoch`.  Evaluation stays `train.evaluate` on the parent graph."""
    if (node_loss is None) == (step_kw is None):
        raise ValueError("give step_kw (GCN / GAT stacks: the keywords of train.train_step) or node_loss (edge-feature stacks)")
    roles = node_roles(loader.g.number_of_nodes(), train_idx, val_idx, test_idx)
    loss_sum, total, skipped = 0.0, 0, 0
    for sub in loader:
        kw = {} if edge_weight is None else {"edge_weight": edge_weight}
        out = subgraph_step(model, sub, optimizer, labels, roles, node_loss=node_loss, step_kw=step_kw, node_mask=node_mask,
                            loss_weight=loss_weight, **kw)
        if out is None:
            skipped += 1
            continue
        loss_sum += float(out[0].detach()) * out[2]
        total += out[2]
    return loss_sum / max(total, 1), skipped
