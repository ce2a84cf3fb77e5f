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

Partition / cluster batches (Cluster-GCN; DGL's `g.subgraph`): `node_subgraph` extracts the subgraph a node set induces on the
device (bot_subgraph_*_i32 in csrc/subgraph.hip) as a `Subgraph` — a square `Graph`, not a block, so the full-batch stacks, the
fused train step and `evaluate()` run on it unchanged; `cluster_assignment` cuts the vertices into parts and `ClusterLoader`
yields one `Subgraph` per group of parts.

GraphSAINT batches (Zeng et al., ICLR 2020; DGL's `SAINTSampler`): `SAINTSampler` picks the node set by short random walks or by
degree-proportional node draws (bot_saint_walk_i32 in csrc/saint.hip, bot_saint_nodes_*_i32 in csrc/sampling.hip) and hands it to
`node_subgraph`; `SAINTLoader` yields the batches of an epoch and `saint_loss_weights` pre-samples the loss normalisation;
`saint_norms` pre-samples the aggregator normalisation with it (per edge C[v] / C[u, v]; bot_subgraph_tally_i32 in csrc/subgraph.hip).

Shared by all of it: `_BatchGraph`, the one constructor of a `Block` and a `Subgraph` (a finished CSC -> `Direction`, row plan, gather
frames, `to()`, and on a GPU the device-built CSR + `csr2csc`: csrc/plan.hip); `_whole_graph`, the guard against blocks and partitions; `_draw_seed`, the 64-bit seed every sampler call takes from
its generator; `_node_map`, the persistent node map; `_SubgraphBatches`, the `__iter__` of the two subgraph loaders.
"""
from __future__ import annotations

import torch

from . import _C
from .graph import Direction, Graph, _Frame, device_plan_enabled, take_rows, xcd_item_order

__all__ = ["MultiLayerNeighborSampler", "MultiLayerFullNeighborSampler", "NodeDataLoader", "Block", "sample_block",
           "Subgraph", "node_subgraph", "cluster_assignment", "ClusterLoader", "SAINTSampler", "SAINTLoader", "saint_loss_weights", "saint_norms"]


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


def _whole_graph(g: Graph, what: str):
    """Mini-batches are cut out of a whole graph: a block or a partition (a graph with a halo plan) raises ValueError."""
    if g.is_block or g.halo is not None:
        raise ValueError(f"{what} takes a whole graph, not a block or a partition")


def _draw_seed(generator):
    """A 64-bit Philox seed from `generator` (torch's default CPU generator if None): one per sampled layer, SAINT batch and
    pre-sampled set."""
    return int(torch.randint(-2 ** 63, 2 ** 63 - 1, (), dtype=torch.int64, generator=generator))


class _BatchGraph(Graph):
    """What a `Block` and a `Subgraph` share: a graph built on the parent's device from a finished CSC - `offsets` [n_dst + 1],
    `local_src` [E] (local source of each edge, rows = destinations, positions ascending in the parent), edge id = CSC position -
    with the row plan of that CSC and frames that gather the parent's rows `node_ids` / `parent_eid` on first access (`parent_rows`: the
    rows of the parent's node tensors behind `node_ids`).  On a GPU the plan, and on first use the CSR with its plan and `csr2csc`, are
    built on the device (csrc/plan.hip: one device->host read of three sizes per direction, one of the transpose's error count); CPU
    tensors, and every graph while `graph.DEVICE_PLAN` is False or BOT_DEVICE_PLAN=0, take the host planner and `build_direction`,
    which give the same arrays."""

    def __init__(self, parent: Graph, n_src, n_dst, offsets, local_src, node_ids, parent_eid):
        E, dev = int(local_src.numel()), node_ids.device
        dst = torch.repeat_interleave(torch.arange(n_dst, device=dev), (offsets[1:] - offsets[:-1]), output_size=E)
        # the edge list is valid by construction: skip Graph's range checks (each one a device->host read)
        empty = torch.empty(0, dtype=torch.int64, device=dev)
        Graph.__init__(self, empty, empty, n_src, num_dst_nodes=n_dst, chunk=parent._chunk)
        local_src = local_src.to(torch.int32).contiguous()
        self._src, self._dst = local_src.long(), dst
        self._src32, self._dst32 = local_src, dst.to(torch.int32).contiguous()
        self.parent_eid = parent_eid
        indptr = offsets.to(torch.int32).contiguous()
        chunk = parent._chunk if parent._chunk is not None else _C.default_chunk(E)
        if indptr.is_cuda and device_plan_enabled():
            items, long_rows, long_ptr, n_slots = _C.row_plan_device(indptr, chunk)                  # one device->host read: three sizes
        else:
            items, long_rows, long_ptr, n_slots = _C.row_plan(indptr.cpu().contiguous(), chunk)      # one device->host copy
        n_long = int(long_rows.numel())
        self._csc = Direction(indptr, local_src, torch.arange(E, dtype=torch.int32, device=dev), items.to(dev),
                              long_rows.to(dev) if n_long else None, long_ptr.to(dev) if n_long else None, n_dst, E,
                              int(items.shape[0]), n_long, n_slots, int(chunk))
        # the parent's node tensors stay in original order: a reordered parent's rows go through its node_perm
        rows = self.parent_rows = node_ids.long() if parent.node_perm is None else parent.node_perm[node_ids.long()]
        self.ndata = _GatherFrame(parent.ndata, lambda x: take_rows(x, rows))
        self.edata = _GatherFrame(parent.edata, lambda x: take_rows(x, parent_eid))

    def to(self, device):
        if torch.device(device) != self.device:
            raise NotImplementedError("blocks and subgraphs are built on the device of their parent graph")
        return self

    @property
    def csr(self) -> Direction:
        """Out-edges grouped by source.  On a GPU: the device transpose of the CSC (edge id = CSC position, so its position array is
        `csr2csc` too) and the device row plan; otherwise `Graph.csr`.  The arrays are the same either way."""
        if self._csr is None:
            csc = self._csc
            if not (csc.indptr.is_cuda and device_plan_enabled()):
                return Graph.csr.fget(self)
            dev = csc.indptr.device
            indptr, indices, eid = _C.csc_transpose(csc.indptr, csc.indices, self._n)
            chunk = self._chunk if self._chunk is not None else _C.default_chunk(csc.nnz)
            items, long_rows, long_ptr, n_slots = _C.row_plan_device(indptr, chunk)
            if self.plan_order == "xcd":
                items = xcd_item_order(items)
            n_long = int(long_rows.numel())
            self._csr = Direction(indptr, indices, eid, items.to(dev), long_rows if n_long else None, long_ptr if n_long else None,
                                  self._n, csc.nnz, int(items.shape[0]), n_long, n_slots, int(chunk), plan_order=self.plan_order)
            self._csr2csc = eid
        return self._csr

    @property
    def csr2csc(self) -> torch.Tensor:
        if self._csr2csc is None:
            _ = self.csr                     # the device transpose leaves csr2csc behind
            if self._csr2csc is None:
                return Graph.csr2csc.fget(self)
        return self._csr2csc


class Block(_BatchGraph):
    """One layer's bipartite message-flow graph of a sampled mini-batch (DGL's block): the sampler's output IS its CSC."""

    def __init__(self, parent: Graph, src_nid, offsets, local_src, parent_eid):
        n_dst = int(offsets.numel()) - 1
        super().__init__(parent, int(src_nid.numel()), n_dst, offsets, local_src, src_nid, parent_eid)
        self.src_nid, self.dst_nid = src_nid, src_nid[:n_dst]
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
    _whole_graph(g, "neighbour sampling")
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
            b = sample_block(g, seeds, fanout, _draw_seed(generator), self.prob)
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


class Subgraph(_BatchGraph):
    """The subgraph of `parent` induced by a node set (DGL's `g.subgraph(nodes)`): a square graph over local ids 0..n-1 (local id =
    position in `parent_nid`), its edges in CSC order (edge id = CSC position) with `parent_eid` (DGL's edata[EID]) and `parent_nid`
    (ndata[NID]).  Degrees, normalisation and the zero-in-degree check are its own.  `ndata` / `edata` gather the parent's rows on
    first access, node rows through the parent's `node_perm` when it was reordered (`parent_rows`: the rows of the parent's
    node tensors, which stay in original order).  Node tensors handed to a stack are in local order (`node_perm` is None).
    The CSC arrays are the extraction kernel's output (`node_subgraph`) or any arrays of that contract, host-built ones included."""

    def __init__(self, parent: Graph, nodes, offsets, local_src, parent_eid):
        n, E = int(nodes.numel()), int(local_src.numel())
        if int(offsets.numel()) != n + 1 or int(parent_eid.numel()) != E:
            raise ValueError("a subgraph's CSC is offsets [n + 1], local_src [E], parent_eid [E]")
        super().__init__(parent, n, n, offsets, local_src, nodes, parent_eid)
        self.parent_nid = nodes


def node_subgraph(g: Graph, nodes) -> Subgraph:
    """`g.subgraph(nodes)`: the subgraph induced by `nodes` — unique ids of `g` (its own ids: internal ones after `reorder_graph`),
    numbered in the order given.  Extraction runs on g's device (csrc/subgraph.hip) with one device->host read; the subgraph's CSR
    and the row plans are built as any batch graph's (`_BatchGraph`: on the device, the CSR lazily; one of each per subgraph, however many
    layers run on it).  Blocks,
    partitioned graphs, duplicates and ids out of range raise ValueError: a node set that arrives from the host is checked there,
    one that is on the device already by the kernel (no extra read)."""
    _whole_graph(g, "an induced subgraph")
    n_nodes = g.number_of_nodes()
    nodes = torch.as_tensor(nodes)
    if nodes.dim() != 1 or nodes.dtype not in (torch.int32, torch.int64):
        raise ValueError("nodes must be a 1-D integer tensor of node ids")
    if not nodes.is_cuda and nodes.numel():
        if int(nodes.min()) < 0 or int(nodes.max()) >= n_nodes:
            raise ValueError(f"node id out of range [0, {n_nodes})")
        if int(torch.unique(nodes).numel()) != int(nodes.numel()):
            raise ValueError("the nodes of a subgraph must be unique")
    nodes = nodes.to(device=g.device, dtype=torch.int32).contiguous()
    offsets, local_src, parent_eid = _C.node_subgraph(g.csc, nodes, _node_map(g))
    return Subgraph(g, nodes, offsets, local_src, parent_eid)


def cluster_assignment(g: Graph, n_parts: int, method: str = "community", seed: int = 0) -> torch.Tensor:
    """int32 [N] on g's device: the part (0 .. n_parts - 1) of every node, parts of equal size (+-1).  "community": the order of
    `reorder_permutation(g, "community")` (vertices grouped by label-propagation label, hubs first inside a label) cut into
    n_parts contiguous ranges; "random": a seeded permutation cut the same way (the baseline: 1 / n_parts of the edges stay inside
    a part).  There is no METIS here: label propagation keeps communities together where the graph has them and cuts through the
    giant label it floods a structureless power-law graph with (graph.label_propagation)."""
    from .graph import reorder_permutation
    n, n_parts = g.number_of_nodes(), int(n_parts)
    _whole_graph(g, "cluster_assignment")
    if not 1 <= n_parts <= max(n, 1):
        raise ValueError(f"n_parts must be in [1, {n}], got {n_parts}")
    if method == "community":
        order = reorder_permutation(g, "community")[0]
    elif method == "random":
        order = torch.randperm(n, generator=torch.Generator().manual_seed(int(seed))).to(g.device)
    else:
        raise ValueError(f"unknown cluster method {method!r}")
    parts = torch.empty(n, dtype=torch.int32, device=g.device)
    parts[order] = ((torch.arange(n, dtype=torch.int64, device=g.device) * n_parts) // max(n, 1)).to(torch.int32)
    return parts


class _SubgraphBatches:
    """`__iter__` of the subgraph loaders: one epoch, the `Subgraph` each node set of `node_batches()` induces on `g`."""

    def __iter__(self):
        for nodes in self.node_batches():
            yield node_subgraph(self.g, nodes)


class ClusterLoader(_SubgraphBatches):
    """Cluster-GCN batches: one epoch per iteration, each batch the `Subgraph` induced by the union of `parts_per_batch` parts of
    `parts` (int [N], a part id per node of `g`, as `cluster_assignment` gives), its nodes in ascending parent id.  The parts are
    dealt in a fresh random order every epoch (`shuffle`), drawn from the loader's own generator: the same seed gives the same
    batches.  `len()` = batches per epoch."""

    def __init__(self, g: Graph, parts, parts_per_batch=1, shuffle=True, seed=0):
        _whole_graph(g, "a cluster loader")
        parts = torch.as_tensor(parts).to(device=g.device, dtype=torch.int64)
        if parts.shape != (g.number_of_nodes(),):
            raise ValueError(f"parts must hold one part id per node ({g.number_of_nodes()}), got {tuple(parts.shape)}")
        if parts.numel() and int(parts.min()) < 0:
            raise ValueError("part ids are non-negative")
        self.g, self.parts_per_batch, self.shuffle = g, int(parts_per_batch), bool(shuffle)
        if self.parts_per_batch < 1:
            raise ValueError("parts_per_batch must be at least 1")
        self.n_parts = int(parts.max()) + 1 if parts.numel() else 0
        self._order = torch.argsort(parts, stable=True).to(torch.int32)          # nodes grouped by part, ascending id inside a part
        self._ptr = [0] + torch.cumsum(torch.bincount(parts, minlength=self.n_parts), 0).tolist()
        self.generator = torch.Generator().manual_seed(int(seed))

    def __len__(self):
        return -(-self.n_parts // self.parts_per_batch)

    def node_batches(self):
        """The node sets of one epoch (int32, ascending parent id), one per batch."""
        order = torch.randperm(self.n_parts, generator=self.generator).tolist() if self.shuffle else list(range(self.n_parts))
        for b in range(len(self)):
            mine = order[b * self.parts_per_batch:(b + 1) * self.parts_per_batch]
            if len(mine) == self.n_parts:                                          # every part: the whole graph, already in order
                yield torch.arange(self.g.number_of_nodes(), dtype=torch.int32, device=self.g.device)
                continue
            pieces = [self._order[self._ptr[p]:self._ptr[p + 1]] for p in mine]
            nodes = pieces[0] if len(pieces) == 1 else torch.sort(torch.cat(pieces)).values
            yield nodes.contiguous()


class SAINTSampler:
    """`dgl.dataloading.SAINTSampler(mode, budget)`: GraphSAINT's node set for one subgraph batch.  mode "walk": `budget` =
    (n_roots, length) - n_roots roots drawn uniformly with replacement from `nids` (g's own ids: internal ones after
    `reorder_graph`; None = every node), from each a walk of `length` steps along uniformly drawn in-edges, the batch = the
    subgraph the visited nodes induce.  mode "node": `budget` = n_draws nodes drawn in proportion to their out-degree, with
    replacement (on a preprocessed, bidirected graph also their in-degree).  The distinct nodes come in ascending id; the draws
    are a pure function of (g, nids, budget, seed) (include/bot_gnn.h).  mode "edge" is not implemented."""

    def __init__(self, mode, budget, nids=None):
        if mode == "edge":
            raise NotImplementedError("GraphSAINT's edge sampler (edges drawn with probability proportional to 1 / deg(u) + 1 / deg(v)) is "
                                      "out of scope: use mode 'walk' or 'node'")
        if mode == "walk":
            self.n_roots, self.length = (int(b) for b in budget)
            self.root_mode = 0
        elif mode == "node":
            if nids is not None:
                raise ValueError("the node sampler draws from every node in proportion to its degree: it takes no nids")
            self.n_roots, self.length, self.root_mode = int(budget), 0, 1
        else:
            raise ValueError(f"unknown SAINT mode {mode!r} ('walk', 'node'; 'edge' is not implemented)")
        if self.n_roots < 0 or self.length < 0:
            raise ValueError(f"budget must be non-negative, got {budget!r}")
        self.mode, self.budget = mode, budget
        self.nids = None if nids is None else torch.as_tensor(nids)
        self._nids_dev = None           # (device, node count the ids were checked against, int32 copy on that device)

    def _nids_on(self, g: Graph):
        if self.nids is None:
            return None
        hit = self._nids_dev
        if hit is None or hit[0] != g.device or hit[1] != g.number_of_nodes():
            nids = self.nids
            if nids.numel() and (int(nids.min()) < 0 or int(nids.max()) >= g.number_of_nodes()):
                raise ValueError("node id out of range")
            hit = self._nids_dev = (g.device, g.number_of_nodes(), nids.to(device=g.device, dtype=torch.int32).contiguous())
        return hit[2]

    def sample_nodes(self, g: Graph, seed: int) -> torch.Tensor:
        """The batch's node set: int32 [n], ascending, on g's device.  One device->host read (n)."""
        _whole_graph(g, "a SAINT node set")
        trace = _C.saint_walk(g.csc, self._nids_on(g), self.n_roots, self.length, self.root_mode, int(seed))
        return _C.saint_nodes(trace, _node_map(g))

    def sample(self, g: Graph, seed: int) -> Subgraph:
        """The batch: `node_subgraph(g, sample_nodes(g, seed))`."""
        return node_subgraph(g, self.sample_nodes(g, seed))


class SAINTLoader(_SubgraphBatches):
    """GraphSAINT batches: one epoch per iteration, `n_batches` `Subgraph`s of `g`, each from `sampler` under a 64-bit seed drawn
    from the loader's own generator (the same `seed` gives the same batches).  `len()` = batches per epoch."""

    def __init__(self, g: Graph, sampler: SAINTSampler, n_batches: int, seed=0):
        _whole_graph(g, "a SAINT loader")
        if int(n_batches) < 1:
            raise ValueError("n_batches must be at least 1")
        self.g, self.sampler, self.n_batches = g, sampler, int(n_batches)
        self.generator = torch.Generator().manual_seed(int(seed))

    def __len__(self):
        return self.n_batches

    def node_batches(self):
        """The node sets of one epoch (int32, ascending parent id), one per batch."""
        for _ in range(self.n_batches):
            yield self.sampler.sample_nodes(self.g, _draw_seed(self.generator))


def saint_loss_weights(g: Graph, sampler: SAINTSampler, n_presample: int, seed=0) -> torch.Tensor:
    """GraphSAINT's loss normalisation, float32 [N] in the parent's ORIGINAL node order (the order of the labels and of
    `minibatch.node_roles`: `lw[sub.parent_rows]` is a batch's slice).  `n_presample` node sets are drawn (`sample_nodes` only, no
    extraction; their seeds from a generator of their own seeded with `seed`), C[v] = the number of sets that hold v, and
    lw[v] = n_presample / max(C[v], 1): the inverse of the estimated probability that a batch holds v.  A pure function of its
    arguments; a host loop of n_presample small launches with one device->host read each."""
    count = _presample(g, sampler, n_presample, seed, None)
    return _loss_weights(g, count, int(n_presample))


def _presample(g: Graph, sampler: SAINTSampler, n_presample, seed, tally):
    """C int32 [N] (g's own ids): the number of the `n_presample` pre-sampled node sets that hold each node; with `tally` (int32 [E],
    zeros, CSC position order) every set is also tallied into it (`_C.subgraph_tally`).  The sets' seeds come from a generator of
    their own seeded with `seed`."""
    n_presample = int(n_presample)
    if n_presample < 1:
        raise ValueError("n_presample must be at least 1")
    gen = torch.Generator().manual_seed(int(seed))
    count = torch.zeros(g.number_of_nodes(), dtype=torch.int32, device=g.device)
    for _ in range(n_presample):
        nodes = sampler.sample_nodes(g, _draw_seed(gen))
        count[nodes.long()] += 1                                            # a set holds no duplicates: no accumulation needed
        if tally is not None:
            _C.subgraph_tally(g.csc, nodes, _node_map(g), tally)
    return count


def _loss_weights(g: Graph, count, n_presample):
    visits = count.clamp(min=1).to(torch.float32)
    lw = torch.full_like(visits, float(n_presample)) / visits              # (tensor / tensor: a true division, correctly rounded)
    if g.node_perm is None:
        return lw
    out = torch.empty_like(lw)
    out[g.node_perm] = lw                                                   # internal id i is original node node_perm[i]
    return out


def saint_norms(g: Graph, sampler: SAINTSampler, n_presample: int, seed=0):
    """GraphSAINT's two normalisations from ONE pre-sampling: (loss_weight, edge_norm).  The `n_presample` node sets are those of
    `saint_loss_weights(g, sampler, n_presample, seed)` (same generator, same seeds) and `loss_weight` is that function's result,
    bit for bit.  edge_norm: float32 [E] in the parent's EDGE-ID order (store it in `g.edata`; a batch gathers its rows through
    `parent_eid`): with C[v] the number of sets that hold v and T[e] the number of sets that induce the edge e = (u -> v), i.e. that
    hold both ends (`_C.subgraph_tally`),
        edge_norm[e] = float32(C[v]) / float32(T[e])   if T[e] > 0,   1.0 otherwise
    (a true division of two integers <= n_presample, which must stay below 2^24).  Multiplied into a batch's aggregation it makes
    the sum over the in-edges of v an unbiased estimate, given that v is in the batch, of the sum over the edges ever induced.
    Consequences: 1 <= edge_norm <= n_presample; a self-loop has weight 1 (T = C[v]); T[e] <= min(C[u], C[v]).
    A pure function of its arguments; per set one more three-launch pass over the set's rows, no extra device->host read."""
    _whole_graph(g, "saint_norms")
    if int(n_presample) >= 2 ** 24:
        raise ValueError("n_presample must stay below 2^24: the counts are divided as float32")
    csc = g.csc
    tally = torch.zeros(csc.nnz, dtype=torch.int32, device=g.device)
    count = _presample(g, sampler, n_presample, seed, tally)
    rows = torch.repeat_interleave(torch.arange(csc.n_rows, device=g.device), (csc.indptr[1:] - csc.indptr[:-1]).long(), output_size=csc.nnz)
    ratio = count[rows].to(torch.float32) / tally.clamp(min=1).to(torch.float32)
    pos = torch.where(tally > 0, ratio, torch.ones((), dtype=torch.float32, device=g.device))
    edge_norm = torch.empty_like(pos)
    edge_norm[csc.eid.long()] = pos
    return _loss_weights(g, count, int(n_presample)), edge_norm
