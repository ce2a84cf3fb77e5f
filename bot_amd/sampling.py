"""Neighbour sampling and mini-batch blocks — the DGL 0.5 surface the reference's ogbn-products / ogbn-proteins scripts train
with (src/ogbn-products/gat.py:196-235, src/ogbn-proteins/gat.py:174-200): `MultiLayerNeighborSampler`,
`MultiLayerFullNeighborSampler`, `NodeDataLoader`.

Sampling runs on the device the parent graph lives on (bot_sample_neighbors_i32, bot_block_mark_i32 / bot_block_relabel_i32 in
csrc/sampling.hip; with `prob`, bot_sample_neighbors_weighted_i32 in csrc/sampling_weighted.hip); there are no worker processes.  A block is a `Graph` with `is_block` true and no halo plan: its
destinations are the first `number_of_dst_nodes()` of its sources, its edges are in CSC order (edge id = CSC position), and it
carries the parent ids of its sources (`src_nid`, DGL's srcdata[NID]) and edges (`parent_eid`, DGL's edata[EID]).  `srcdata` /
`edata` gather the parent's `ndata` / `edata` rows on first access; `dstdata` is a frame of its own over the destination prefix.

Ids are the parent graph's own ids (after `reorder_graph`: internal ids; the node features, kept in original order, are
gathered through `node_perm`).
"""
from __future__ import annotations

import torch

from . import _C
from .graph import Direction, Graph, _Frame, build_direction, take_rows

__all__ = ["MultiLayerNeighborSampler", "MultiLayerFullNeighborSampler", "NodeDataLoader", "Block", "sample_block"]


class _GatherFrame(_Frame):
    """A feature frame whose rows are `source[key][index]`, gathered on first access (writes are local to this frame)."""

    def __init__(self, source, index):
        super().__init__()
        self._source, self._index = source, index

    def _load(self, key):
        if not dict.__contains__(self, key) and key in self._source:
            dict.__setitem__(self, key, self._index(self._source[key]))

    def __getitem__(self, key):
        self._load(key)
        return dict.__getitem__(self, key)

    def get(self, key, default=None):
        self._load(key)
        return dict.get(self, key, default)

    def __contains__(self, key):
        return dict.__contains__(self, key) or key in self._source

    def keys(self):
        return list(dict.keys(self)) + [k for k in self._source if not dict.__contains__(self, k)]

    def __iter__(self):
        return iter(self.keys())

    def __len__(self):
        return len(self.keys())

    def items(self):
        return [(k, self[k]) for k in self.keys()]

    def values(self):
        return [self[k] for k in self.keys()]


class Block(Graph):
    """One layer's bipartite message-flow graph of a sampled mini-batch (DGL's block)."""

    def __init__(self, parent: Graph, src_nid, offsets, local_src, parent_eid):
        n_src, n_dst, E = int(src_nid.numel()), int(offsets.numel()) - 1, int(local_src.numel())
        dev = src_nid.device
        dst = torch.repeat_interleave(torch.arange(n_dst, device=dev), (offsets[1:] - offsets[:-1]), output_size=E)
        # the edge list is valid by construction: skip Graph's range checks (each one a device->host read)
        Graph.__init__(self, torch.empty(0, dtype=torch.int64, device=dev), torch.empty(0, dtype=torch.int64, device=dev), n_src,
                       num_dst_nodes=n_dst, chunk=parent._chunk)
        self._src, self._dst = local_src.long(), dst
        self._src32, self._dst32 = local_src, dst.to(torch.int32).contiguous()
        self.src_nid, self.dst_nid, self.parent_eid = src_nid, src_nid[:n_dst], parent_eid
        indptr = offsets.to(torch.int32).contiguous()
        chunk = parent._chunk if parent._chunk is not None else _C.default_chunk(E)
        items, long_rows, long_ptr, n_slots = _C.row_plan(indptr.cpu().contiguous(), chunk)      # one device->host copy
        n_long = int(long_rows.numel())
        # the sampler's output IS the block's CSC: rows = destinations, positions ascending in the parent, edge id = position
        self._csc = Direction(indptr, local_src, torch.arange(E, dtype=torch.int32, device=dev), items.to(dev),
                              long_rows.to(dev) if n_long else None, long_ptr.to(dev) if n_long else None, n_dst, E,
                              int(items.shape[0]), n_long, n_slots, int(chunk))
        node_rows = src_nid.long() if parent.node_perm is None else parent.node_perm[src_nid.long()]
        self.ndata = _GatherFrame(parent.ndata, lambda x: take_rows(x, node_rows))
        self.edata = _GatherFrame(parent.edata, lambda x: take_rows(x, parent_eid))
        self._dstdata = _GatherFrame(self.ndata, lambda x: x[:n_dst])

    @property
    def is_block(self):
        return True

    @property
    def dstdata(self):
        return self._dstdata

    def extend(self, x_src):
        """Source rows are what the layer holds already (feat_src has number_of_src_nodes() rows)."""
        if x_src.shape[0] != self._n:
            raise ValueError(f"a sampled block takes features of its {self._n} source nodes, got {x_src.shape[0]} rows")
        return x_src

    def to(self, device):
        if torch.device(device) != self.device:
            raise NotImplementedError("blocks are built on the device of their parent graph")
        return self


def _node_map(g: Graph):
    """The persistent int32 map over the parent's nodes that to_block works in (all -1 between calls)."""
    m = getattr(g, "_bot_block_map", None)
    if m is None or m.device != g.device:
        m = g._bot_block_map = torch.full((g.number_of_nodes(),), -1, dtype=torch.int32, device=g.device)
    return m


def _prepared_weights(g: Graph, prob):
    """The prepared form of the edge weights `prob` (an edata key or a float32 [E] / [E, 1] tensor) for weighted sampling, cached
    on the parent graph under (key, data_ptr, _version): an in-place change of the weights is seen, and one weight tensor is
    kept at a time (8 B per edge)."""
    w = g.edata[prob] if isinstance(prob, str) else prob
    if not isinstance(w, torch.Tensor):
        raise TypeError(f"prob must be an edata key or a tensor, got {type(prob).__name__}")
    key = (prob if isinstance(prob, str) else None, w.data_ptr(), w._version, tuple(w.shape), w.device)
    hit = getattr(g, "_bot_prob_cache", None)
    if hit is not None and hit[0] == key:
        return hit[1]
    g._bot_prob_cache = None                       # drop the old prefix before allocating the new one
    prepared = _C.sample_weights_prepare(g.csc, w)
    g._bot_prob_cache = (key, prepared)
    return prepared


def sample_block(g: Graph, seeds: torch.Tensor, fanout: int, seed: int, prob=None) -> Block:
    """`to_block(sample_neighbors(g, seeds, fanout, prob=prob))` in one: the block whose destinations are `seeds` (unique parent
    ids, int32 on g's device) and whose edges are min(deg, fanout) in-edges of each, uniformly without replacement; with `prob`
    (an edata key or a per-edge weight tensor) min(n_pos, fanout) in-edges, drawn in proportion to their weights without
    replacement (include/bot_gnn.h), n_pos = the number of in-edges of positive weight."""
    if g.is_block or g.halo is not None:
        raise ValueError("neighbour sampling runs on a whole graph")
    csc = g.csc
    if prob is None:
        offsets, pos = _C.sample_neighbors(csc, seeds, fanout, seed)
    else:
        offsets, pos = _C.sample_neighbors_weighted(csc, _prepared_weights(g, prob), seeds, fanout, seed)
    src_nid, local, parent_eid = _C.block_relabel(csc, seeds, pos, _node_map(g))
    return Block(g, src_nid, offsets, local, parent_eid)


class MultiLayerNeighborSampler:
    """`dgl.dataloading.MultiLayerNeighborSampler(fanouts, prob=None)`: fanouts[i] in-edges per destination for layer i (-1: all),
    uniformly, or with `prob` (an edata key of the parent graph or a per-edge weight tensor) in proportion to the edge weights."""

    def __init__(self, fanouts, replace=False, return_eids=False, prob=None):
        if replace:
            raise NotImplementedError("sampling with replacement is not implemented (the reference samples without)")
        if prob is not None and not isinstance(prob, (str, torch.Tensor)):
            raise TypeError(f"prob must be an edata key or a tensor, got {type(prob).__name__}")
        self.fanouts = [int(f) for f in fanouts]
        self.prob = prob

    def sample_blocks(self, g: Graph, seed_nodes: torch.Tensor, generator: torch.Generator | None = None):
        """Blocks from the input layer to the output layer; blocks[-1]'s destinations are `seed_nodes`.  Each layer's 64-bit
        Philox seed is drawn from `generator` (torch's default CPU generator if None)."""
        seeds = seed_nodes.to(device=g.device, dtype=torch.int32).contiguous()
        blocks = []
        for fanout in reversed(self.fanouts):
            s = int(torch.randint(-2 ** 63, 2 ** 63 - 1, (), dtype=torch.int64, generator=generator))
            b = sample_block(g, seeds, fanout, s, self.prob)
            blocks.insert(0, b)
            seeds = b.src_nid
        return blocks


class MultiLayerFullNeighborSampler(MultiLayerNeighborSampler):
    """`dgl.dataloading.MultiLayerFullNeighborSampler(n_layers)`: every in-edge, every layer."""

    def __init__(self, n_layers, return_eids=False):
        super().__init__([-1] * int(n_layers))


class NodeDataLoader:
    """`dgl.dataloading.NodeDataLoader(g, nids, sampler, batch_size=..., shuffle=..., drop_last=...)`: one epoch per iteration,
    yielding (input_nodes, output_nodes, blocks) with input_nodes = blocks[0].src_nid and output_nodes = blocks[-1].dst_nid
    (int64).  `seed` seeds the loader's own generator (the shuffle and the per-layer sampling seeds): the same seed gives the same
    batches.  The reference's `batch_sampler=BatchSampler(n, batch_size, shuffle)` maps onto batch_size / shuffle."""

    def __init__(self, g: Graph, nids, sampler, batch_size=1, shuffle=False, drop_last=False, seed=0, **unused):
        self.g, self.sampler = g, sampler
        self.nids = torch.as_tensor(nids).to(device=g.device, dtype=torch.int64)
        if self.nids.numel() and (int(self.nids.min()) < 0 or int(self.nids.max()) >= g.number_of_nodes()):
            raise ValueError("node id out of range")
        self.batch_size, self.shuffle, self.drop_last = int(batch_size), bool(shuffle), bool(drop_last)
        self.generator = torch.Generator().manual_seed(int(seed))

    def __len__(self):
        n = int(self.nids.numel())
        return n // self.batch_size if self.drop_last else -(-n // self.batch_size)

    def __iter__(self):
        n = int(self.nids.numel())
        order = torch.randperm(n, generator=self.generator).to(self.nids.device) if self.shuffle else None
        for b in range(len(self)):
            lo, hi = b * self.batch_size, min(n, (b + 1) * self.batch_size)
            out = self.nids[lo:hi] if order is None else self.nids[order[lo:hi]]
            blocks = self.sampler.sample_blocks(self.g, out, self.generator)
            yield blocks[0].src_nid.long(), out, blocks
