"""Mini-batch training and evaluation over sampled blocks — the loops of src/ogbn-products/gat.py:113-193 and
src/ogbn-proteins/gat.py:96-171, on `bot_amd.sampling.NodeDataLoader` batches."""
from __future__ import annotations

import torch

__all__ = ["add_labels", "train_epoch", "evaluate"]


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
