"""Graph object for full-batch message passing on one MI355X.

Mirrors the closed slice of the `dgl 0.5.*` graph surface that the reference layers touch
(reference src/no-sampling/models.py:333-388, 476-551; run.py:138-146) so the
reference's layer code runs on it unchanged, and holds the device-side structures the HIP kernels
consume: both compressed directions (in-edges by destination = "csc", out-edges by source = "csr"),
int32, each stable in edge id, with the position->edge-id permutations and the row plans.
"""
from __future__ import annotations

import contextlib
import os
from dataclasses import dataclass

import torch

from . import _C

_TAKE_CHUNK = 1 << 24

# Mini-batch graphs (bot_amd.sampling._BatchGraph) on a GPU build their row plans and their CSR on the device (csrc/plan.hip); False, or
# BOT_DEVICE_PLAN=0 in the environment, selects the host planner and `build_direction`.  Both are read at call time.
DEVICE_PLAN = True


def device_plan_enabled() -> bool:
    return bool(DEVICE_PLAN) and os.environ.get("BOT_DEVICE_PLAN", "1") != "0"


def take_rows(x: torch.Tensor, idx: torch.Tensor) -> torch.Tensor:
    """`x[idx]` along dim 0 for index tensors of any length.  torch-ROCm 2.10's row gather returns wrong rows (or raises
    hipErrorInvalidConfiguration) from 2^26 indices on when a row is 16 bytes — measured on S-products / S-proteins edge
    tensors, tools/exp_torch_large.py — so edge-sized gathers go through here: pieces of 2^24 indices into one output buffer."""
    idx = idx.long()
    if idx.numel() <= _TAKE_CHUNK:
        return x[idx]
    out = torch.empty((idx.numel(),) + tuple(x.shape[1:]), dtype=x.dtype, device=x.device)
    for a in range(0, idx.numel(), _TAKE_CHUNK):
        torch.index_select(x, 0, idx[a:a + _TAKE_CHUNK], out=out[a:a + _TAKE_CHUNK])
    return out


@dataclass
class Direction:
    """One compressed direction + its row plan (include/bot_gnn.h "Row plan")."""
    indptr: torch.Tensor     # int32 [n_rows+1]
    indices: torch.Tensor    # int32 [nnz]  neighbour node of each position
    eid: torch.Tensor        # int32 [nnz]  position -> edge id
    items: torch.Tensor      # int32 [n_items,4]
    long_rows: torch.Tensor | None
    long_ptr: torch.Tensor | None
    n_rows: int
    nnz: int
    n_items: int
    n_long: int
    n_slots: int
    chunk: int
    blocked: dict = None     # row width -> bot_amd.blocked.BlockedPlan (dense graphs; built lazily on the device)
    plan_order: str = "degree"   # item order of the plan: "degree" (longest first) or "xcd" (xcd_item_order: the numbering has locality)

    def __post_init__(self):
        if self.blocked is None:
            self.blocked = {}

    def to(self, device):
        mv = lambda t: None if t is None else t.to(device)
        return Direction(mv(self.indptr), mv(self.indices), mv(self.eid), mv(self.items), mv(self.long_rows),
                         mv(self.long_ptr), self.n_rows, self.nnz, self.n_items, self.n_long, self.n_slots, self.chunk,
                         plan_order=self.plan_order)


def xcd_item_order(items: torch.Tensor) -> torch.Tensor:
    """Row-plan items re-ordered for graphs whose NUMBERING carries locality (after `reorder_graph`): workgroups are dealt
    round-robin over the 8 XCDs (block b and b + 8 share an L2, MI355X_MICROARCH.md "Workgroup dispatch"), a workgroup is 4
    wavefronts = 4 items, so the whole-row items are cut into 8 contiguous row ranges and dealt 4 at a time, range x to the
    blocks with b % 8 == x.  Each XCD then sweeps ITS range of rows in order, and rows that share sources (a community) are
    gathered through one L2 at about the same time.  The chunks of long rows stay in front (they start first).  A pure
    re-ordering: every item appears exactly once, results are unchanged.  Placement is a speed heuristic only."""
    whole = items[:, 3] < 0
    longs, rest = items[~whole], items[whole]
    rest = rest[torch.argsort(rest[:, 0], stable=True)]                      # natural row order
    lead = (-longs.shape[0]) % 4                                             # keep 4-item groups aligned with workgroups
    head, rest = rest[:lead], rest[lead:]
    n = rest.shape[0]
    if n:
        seg = ((n + 7) // 8 + 3) // 4 * 4                                    # rows per XCD range, a multiple of 4
        q = torch.arange(n, device=items.device)
        x, o = q // seg, q % seg
        rest = rest[torch.argsort((o // 4) * 32 + x * 4 + o % 4, stable=True)]
    return torch.cat([longs, head, rest]).contiguous()


def build_direction(rows: torch.Tensor, cols: torch.Tensor, n_rows: int, chunk: int | None = None, order: str = "degree") -> Direction:
    """Compress the COO list (edge e: row rows[e], neighbour cols[e]) by row, stable in edge id.

    Integer work done with torch on whatever device the edge list lives on; the row plan is host-side C.
    `order`: "degree" = the plan's longest-first item order; "xcd" = `xcd_item_order`.
    """
    dev = rows.device
    nnz = int(rows.numel())
    if nnz >= 2 ** 31 - 1 or n_rows >= 2 ** 31 - 1:
        raise ValueError("bot_amd uses int32 indices: graph too large")
    eid = torch.argsort(rows, stable=True)
    counts = torch.bincount(rows, minlength=n_rows)
    indptr = torch.zeros(n_rows + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(counts, 0)
    indptr32 = indptr.to(torch.int32)
    if chunk is None:
        chunk = _C.default_chunk(nnz)
    items, long_rows, long_ptr, n_slots = _C.row_plan(indptr32.cpu().contiguous(), chunk)
    if order == "xcd":
        items = xcd_item_order(items)
    n_long = int(long_rows.numel())
    return Direction(indptr32.contiguous(), take_rows(cols, eid).to(torch.int32).contiguous(), eid.to(torch.int32).contiguous(),
                     items.to(dev), long_rows.to(dev) if n_long else None, long_ptr.to(dev) if n_long else None,
                     int(n_rows), nnz, int(items.shape[0]), n_long, n_slots, int(chunk), plan_order=order)


def sub_direction(d: Direction, positions: torch.Tensor, index_offset: int = 0) -> tuple:
    """The compressed direction made of the given POSITIONS of `d` (ascending; same rows, same order inside a row) with its own row
    plan, plus `positions` as int32 — the `wperm` / `operm` through which a kernel on the sub-direction reaches arrays laid out in
    `d`'s position order (attention weights, per-edge dot products).  `index_offset` is subtracted from the neighbour ids (a table
    that holds only the halo rows).  Integer work on the device of `d`."""
    dev = d.indptr.device
    pos = positions.long()
    deg = (d.indptr[1:] - d.indptr[:-1]).long()
    row_of = torch.repeat_interleave(torch.arange(d.n_rows, device=dev), deg)
    counts = torch.bincount(row_of[pos], minlength=d.n_rows)
    indptr = torch.zeros(d.n_rows + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(counts, 0)
    indptr32 = indptr.to(torch.int32).contiguous()
    items, long_rows, long_ptr, n_slots = _C.row_plan(indptr32.cpu().contiguous(), d.chunk)
    n_long = int(long_rows.numel())
    sub = Direction(indptr32, (take_rows(d.indices, pos) - index_offset).to(torch.int32).contiguous(), take_rows(d.eid, pos).contiguous(),
                    items.to(dev), long_rows.to(dev) if n_long else None, long_ptr.to(dev) if n_long else None, d.n_rows,
                    int(pos.numel()), int(items.shape[0]), n_long, n_slots, d.chunk, plan_order="degree")
    return sub, pos.to(torch.int32).contiguous()


def row_range_direction(d: Direction, lo: int, hi: int) -> tuple:
    """Rows [lo, hi) of `d` as a direction of its own (rows renumbered from 0, neighbour ids unchanged) and the int32 positions of its
    entries in `d` — the rows are contiguous, so this is a slice."""
    dev = d.indptr.device
    a, b = int(d.indptr[lo]), int(d.indptr[hi])
    indptr32 = (d.indptr[lo:hi + 1] - a).to(torch.int32).contiguous()
    items, long_rows, long_ptr, n_slots = _C.row_plan(indptr32.cpu().contiguous(), d.chunk)
    n_long = int(long_rows.numel())
    sub = Direction(indptr32, d.indices[a:b].contiguous(), d.eid[a:b].contiguous(), items.to(dev), long_rows.to(dev) if n_long else None,
                    long_ptr.to(dev) if n_long else None, hi - lo, b - a, int(items.shape[0]), n_long, n_slots, d.chunk, plan_order="degree")
    return sub, torch.arange(a, b, dtype=torch.int32, device=dev)


class _Frame(dict):
    """Feature dict (`graph.ndata` / `graph.edata`)."""


class Graph:
    """Graph over nodes 0..N-1 with edges in edge-id order (edge e: src[e] -> dst[e]).

    With `num_dst_nodes < num_nodes` it is a *block* in DGL's sense (models.py:493-496): destinations
    are the first `num_dst_nodes` source nodes.  The 1-D vertex-partitioned mode uses exactly that
    shape — owned vertices first, halo sources appended (bot_amd/dist.py) — and may attach a `halo`
    plan that extends owned node features with the remote rows (`Graph.extend`)."""

    def __init__(self, src, dst, num_nodes: int, *, num_dst_nodes: int | None = None, chunk: int | None = None):
        src = torch.as_tensor(src).to(torch.int64)
        dst = torch.as_tensor(dst).to(torch.int64)
        if src.shape != dst.shape or src.dim() != 1:
            raise ValueError("src and dst must be 1-D tensors of equal length")
        n_dst = int(num_nodes if num_dst_nodes is None else num_dst_nodes)
        if n_dst > num_nodes:
            raise ValueError("num_dst_nodes exceeds num_nodes")
        if src.numel() and (int(src.max()) >= num_nodes or int(dst.max()) >= n_dst or int(torch.min(src.min(), dst.min())) < 0):
            raise ValueError("node id out of range")
        self._src, self._dst, self._n, self._n_dst = src, dst, int(num_nodes), n_dst
        self._chunk = chunk
        self.plan_order = "degree"       # item order of the row plans (build_direction)
        # set by `reorder_graph`: this graph's ids are INTERNAL ids; node_perm[new] = original id, node_inv[original] = new.
        # The stacks (bot_amd.nn.GCN / GAT / edge GATs) take and return node tensors in ORIGINAL order and convert at their
        # boundary (to_internal / to_original); the operator-level surface (update_all, ops.*) works in the graph's own ids.
        self.node_perm = self.node_inv = None
        self.halo = None                 # bot_amd.dist.HaloPlan in partitioned mode
        self.global_out_degrees = None   # int64 [num_dst_nodes]: out-degrees in the WHOLE graph (partitioned mode)
        self._csc = self._csr = self._csr2csc = self._csc2csr = None
        self._src32 = self._dst32 = None
        self._halo_split = None
        self.ndata, self.edata = _Frame(), _Frame()

    # ---------------------------------------------------------------- dgl-like queries
    @property
    def device(self):
        return self._src.device

    @property
    def is_block(self):
        return self._n_dst != self._n

    def extend(self, x_dst):
        """Owned/destination node features -> source node features.  Identity on a full graph; in
        partitioned mode appends the halo rows fetched from their owners (RCCL all-to-all)."""
        if self.halo is not None:
            return self.halo.extend(x_dst)
        if self.is_block:
            raise ValueError("a block without a halo plan needs source features supplied by the caller")
        return x_dst

    def to_internal(self, x):
        """Node tensor in original order -> the order of this graph's ids (identity unless `reorder_graph` made this graph)."""
        return x if self.node_perm is None else x.index_select(0, self.node_perm)

    def to_original(self, y):
        """Node tensor in this graph's ids -> original order."""
        return y if self.node_inv is None else y.index_select(0, self.node_inv)

    @property
    def srcdata(self):
        return self.ndata

    @property
    def dstdata(self):
        return self.ndata

    def number_of_nodes(self):
        return self._n

    num_nodes = number_of_nodes

    def number_of_src_nodes(self):
        return self._n

    def number_of_dst_nodes(self):
        return self._n_dst

    def number_of_edges(self):
        return int(self._src.numel())

    num_edges = number_of_edges

    def edges(self):
        return self._src, self._dst

    def in_degrees(self):
        """int64 [N] — models.py:335,388,478,551.  Computed by the HIP degree kernel from the CSC row pointer."""
        return _C.degrees(self.csc)

    def out_degrees(self):
        """int64 [N] — models.py:352,501; ogbn-proteins/gat.py:64."""
        return _C.degrees(self.csr)

    @contextlib.contextmanager
    def local_scope(self):
        """models.py:333,476 — feature writes inside the scope do not leak out."""
        nd, ed = _Frame(self.ndata), _Frame(self.edata)
        try:
            yield
        finally:
            self.ndata, self.edata = nd, ed

    def to(self, device):
        device = torch.device(device)
        if device == self.device:
            return self
        g = Graph(self._src.to(device), self._dst.to(device), self._n, num_dst_nodes=self._n_dst, chunk=self._chunk)
        g.plan_order = self.plan_order
        for name in ("_csc", "_csr", "_csr2csc", "_csc2csr", "_src32", "_dst32", "global_out_degrees", "halo", "node_perm", "node_inv"):
            v = getattr(self, name)
            setattr(g, name, None if v is None else v.to(device))
        g.ndata = _Frame({k: v.to(device) for k, v in self.ndata.items()})
        g.edata = _Frame({k: v.to(device) for k, v in self.edata.items()})
        return g

    def create_formats_(self):
        """run.py:146 — materialise both compressed directions now."""
        _ = self.csc, self.csr, self.csr2csc
        return None

    # ---------------------------------------------------------------- transforms (run.py:138-143); integer, bit-exact
    def remove_self_loop(self):
        assert not self.is_block, "graph transforms apply to whole graphs"
        keep = self._src != self._dst
        g = Graph(self._src[keep], self._dst[keep], self._n, chunk=self._chunk)
        g.ndata = _Frame(self.ndata)
        return g

    def add_self_loop(self):
        assert not self.is_block, "graph transforms apply to whole graphs"
        loops = torch.arange(self._n, dtype=torch.int64, device=self.device)
        g = Graph(torch.cat([self._src, loops]), torch.cat([self._dst, loops]), self._n, chunk=self._chunk)
        g.ndata = _Frame(self.ndata)
        return g

    def subgraph(self, nodes):
        """`dgl.DGLGraph.subgraph(nodes)`: the subgraph induced by `nodes` (bot_amd.sampling.node_subgraph)."""
        from .sampling import node_subgraph
        return node_subgraph(self, nodes)

    # ---------------------------------------------------------------- device structures
    @property
    def csc(self) -> Direction:
        """In-edges grouped by destination: rows = dst, indices = src."""
        if self._csc is None:
            self._csc = build_direction(self._dst, self._src, self._n_dst, self._chunk, self.plan_order)
        return self._csc

    @property
    def csr(self) -> Direction:
        """Out-edges grouped by source: rows = src, indices = dst."""
        if self._csr is None:
            self._csr = build_direction(self._src, self._dst, self._n, self._chunk, self.plan_order)
        return self._csr

    def _inverse(self, perm):
        inv = torch.empty_like(perm)
        inv[perm.long()] = torch.arange(perm.numel(), dtype=perm.dtype, device=perm.device)
        return inv

    @property
    def csr2csc(self) -> torch.Tensor:
        """int32 [E]: CSC position of the edge that sits at CSR position k."""
        if self._csr2csc is None:
            self._csr2csc = take_rows(self._inverse(self.csc.eid), self.csr.eid).contiguous()
        return self._csr2csc

    @property
    def halo_split(self):
        """Partitioned blocks (owned vertices first, halo sources behind): the structures that let a layer work on the edges whose
        source is OWNED while the halo rows are still in flight, and finish with the halo-source edges afterwards —
          csc_own / csc_halo   in-edges split by source class (csc_halo's neighbour ids index the halo table alone), with the
                               positions of their entries in `csc` (the order the attention weights are kept in);
          csr_own / csr_halo   out-edges of the owned rows / of the halo rows (rows renumbered from 0), with the CSC position of
                               every entry (csr2csc restricted to them).
        Per destination the sum then runs over the owned-source edges first and the halo-source edges second (each in edge-id
        order) — not the single-GPU order, by design; values agree to rounding, not bitwise."""
        if self._halo_split is None:
            assert self.halo is not None, "halo_split applies to the blocks of a partition"   # (a 1-rank partition has no halo rows)
            n_own = self._n_dst
            csc, csr = self.csc, self.csr
            own_pos = torch.nonzero(csc.indices < n_own).squeeze(1)
            halo_pos = torch.nonzero(csc.indices >= n_own).squeeze(1)
            csc_own, p_own = sub_direction(csc, own_pos)
            csc_halo, p_halo = sub_direction(csc, halo_pos, index_offset=n_own)
            csr_own, q_own = row_range_direction(csr, 0, n_own)
            csr_halo, q_halo = row_range_direction(csr, n_own, self._n)
            c2c = self.csr2csc
            self._halo_split = dict(csc_own=csc_own, csc_own_pos=p_own, csc_halo=csc_halo, csc_halo_pos=p_halo,
                                    csr_own=csr_own, csr_own_c2c=take_rows(c2c, q_own.long()).contiguous(),
                                    csr_halo=csr_halo, csr_halo_c2c=take_rows(c2c, q_halo.long()).contiguous())
        return self._halo_split

    @property
    def src32(self):
        if self._src32 is None:
            self._src32 = self._src.to(torch.int32).contiguous()
        return self._src32

    @property
    def dst32(self):
        if self._dst32 is None:
            self._dst32 = self._dst.to(torch.int32).contiguous()
        return self._dst32

    # ---------------------------------------------------------------- message passing (dgl.function builders)
    def apply_edges(self, msg):
        """models.py:523,525 — `fn.u_add_v` / `fn.copy_u` into edata."""
        from . import ops
        if msg.kind == "copy_u":
            self.edata[msg.out] = ops.copy_u(self, self.ndata[msg.a])
        elif msg.kind == "u_add_v":
            self.edata[msg.out] = ops.u_add_v(self, self.ndata[msg.a], self.ndata[msg.b])
        else:
            raise NotImplementedError(f"apply_edges({msg.kind})")

    def update_all(self, msg, reduce):
        """models.py:374,381,547; ogbn-proteins/gat.py:58 — (copy_u | u_mul_e | copy_e) + sum; (copy_u | u_mul_e) + mean: the sum
        times 1 / in_degree (0 for a node without in-edges); copy_u + max / min: the element-wise max / min (`ops.copy_u_max`, `ops.copy_u_min`; 0 for such a node)."""
        from . import ops
        if reduce.kind not in ("sum", "max", "min", "mean") or reduce.msg != msg.out:
            raise NotImplementedError("only fn.sum / fn.max / fn.min / fn.mean over the message field are supported")
        if reduce.kind == "min":
            if msg.kind != "copy_u":
                raise NotImplementedError(f"update_all({msg.kind}, min): the min reducer takes fn.copy_u messages only (the sweep "
                                          "gathers source rows; it has no per-edge factor)")
            self.ndata[reduce.out] = ops.copy_u_min(self, self.ndata[msg.a])
            return
        if reduce.kind == "max":
            if msg.kind != "copy_u":
                raise NotImplementedError(f"update_all({msg.kind}, max): the max reducer takes fn.copy_u messages only (the max kernel "
                                          "gathers source rows; it has no per-edge factor)")
            self.ndata[reduce.out] = ops.copy_u_max(self, self.ndata[msg.a])
            return
        if reduce.kind == "mean" and msg.kind not in ("copy_u", "u_mul_e"):
            raise NotImplementedError(f"update_all({msg.kind}, mean)")
        if msg.kind == "copy_u":
            out = ops.copy_u_sum(self, self.ndata[msg.a])
        elif msg.kind == "u_mul_e":
            out = ops.u_mul_e_sum(self, self.ndata[msg.a], self.edata[msg.b])
        elif msg.kind == "copy_e":
            out = ops.copy_e_sum(self, self.edata[msg.a])
        else:
            raise NotImplementedError(f"update_all({msg.kind})")
        if reduce.kind == "mean":
            deg = self.in_degrees().to(out.dtype)
            inv = torch.where(deg > 0, 1.0 / deg.clamp(min=1), torch.zeros_like(deg))
            out = out * inv.reshape((-1,) + (1,) * (out.dim() - 1))
        self.ndata[reduce.out] = out


def graph(edges, num_nodes=None) -> Graph:
    """`dgl.graph((src, dst))` (models.py:187)."""
    src, dst = (torch.as_tensor(x).to(torch.int64) for x in edges)
    if num_nodes is None:
        num_nodes = int(torch.max(src.max(), dst.max())) + 1 if src.numel() else 0
    return Graph(src, dst, num_nodes)


def to_bidirected(g: Graph) -> Graph:
    """`dgl.to_bidirected(graph)` — run.py:138.  Adds every reverse edge, then collapses duplicate
    (src, dst) pairs; the result is ordered by (src, dst).  Node/edge features are dropped (the
    reference re-attaches `feat` itself, run.py:137-139).  Integer work, bit-exact vs the oracle."""
    n = g.number_of_nodes()
    key = torch.unique(torch.cat([g._src * n + g._dst, g._dst * n + g._src]))
    return Graph(torch.div(key, n, rounding_mode="floor"), key % n, n, chunk=g._chunk)


def add_self_loop(g: Graph) -> Graph:
    return g.add_self_loop()


def remove_self_loop(g: Graph) -> Graph:
    return g.remove_self_loop()


def label_propagation(src, dst, n: int, iters: int = 10) -> torch.Tensor:
    """A cheap community pass, entirely with device-side integer ops (sort / unique / scatter-reduce): every vertex starts
    in its own community and repeatedly adopts the label most frequent among its in-neighbours (ties: the smallest label);
    half of the vertices (a hash of the id, alternating) move per sweep, which keeps the synchronous form from oscillating.
    O(E log E) per sweep.  On a graph with planted blocks it recovers them within ~10 sweeps (87 % of the edges inside a
    label at p_in = 0.9); on a structureless power-law graph the labels flood into one giant community — harmless for the use
    made of them here (an ORDER: vertices grouped by label, hubs first inside a label)."""
    dev = src.device
    labels = torch.arange(n, dtype=torch.int64, device=dev)
    ids = torch.arange(n, dtype=torch.int64, device=dev)
    for it in range(iters):
        key = torch.sort(dst * n + labels[src]).values
        uniq, counts = torch.unique_consecutive(key, return_counts=True)
        du, lu = torch.div(uniq, n, rounding_mode="floor"), uniq % n
        best = torch.zeros(n, dtype=counts.dtype, device=dev).scatter_reduce(0, du, counts, "amax")
        cand = torch.where(counts == best[du], lu, torch.full_like(lu, n))
        new = torch.full((n,), n, dtype=torch.int64, device=dev).scatter_reduce(0, du, cand, "amin")
        new = torch.where(new == n, labels, new)                       # no in-edges: keep
        move = (((ids * 2654435761) >> 7) + it) % 2 == 0
        labels = torch.where(move, new, labels)
    return labels


def reorder_permutation(g: Graph, method: str = "community"):
    """(perm [N] int64: new id -> old id, labels or None).  "degree": in-degree descending (stable in the old id);
    "community": grouped by `label_propagation` label (communities in order of their smallest member), in-degree descending
    inside a community."""
    n = g.number_of_nodes()
    src, dst = g.edges()
    deg = torch.bincount(dst, minlength=n)
    if method == "degree":
        return torch.argsort(deg, descending=True, stable=True), None
    if method != "community":
        raise ValueError(f"unknown reorder method {method!r}")
    labels = label_propagation(src, dst, n)
    by_deg = torch.argsort(deg, descending=True, stable=True)
    return by_deg[torch.argsort(labels[by_deg], stable=True)], labels


def reorder_graph(g: Graph, method: str = "community", plan_order: str | None = None) -> Graph:
    """The same graph under a locality-friendly vertex numbering.  Edge e keeps its id and its endpoints
    (relabelled), so per-destination sums run over the same edges in the same order and every integer property (degrees,
    edge ids, CSC/CSR contents) maps back through `node_perm` exactly; node tensors handed to / returned by the stacks stay
    in ORIGINAL order (`to_internal` / `to_original`).  With method="community" and a real community structure (no label
    holding over a quarter of the vertices) the row plans use the XCD-aware item order; `plan_order` ("degree" | "xcd")
    overrides that choice (the item order never changes a result, only where a row is swept)."""
    assert not g.is_block, "reorder applies to whole graphs"
    perm, labels = reorder_permutation(g, method)
    n = g.number_of_nodes()
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(n, dtype=perm.dtype, device=perm.device)
    s, d = g.edges()
    h = Graph(inv[s], inv[d], n, chunk=g._chunk)
    h.node_perm, h.node_inv = perm, inv
    h.ndata, h.edata = _Frame(g.ndata), _Frame(g.edata)                 # frames stay in original node / edge order
    if plan_order is not None:
        if plan_order not in ("degree", "xcd"):
            raise ValueError(f"unknown plan order {plan_order!r}")
        h.plan_order = plan_order
    elif labels is not None and int(torch.bincount(labels).max()) * 4 <= n:
        h.plan_order = "xcd"
    return h


def preprocess(g: Graph, reorder: str | None = None, plan_order: str | None = None) -> Graph:
    """The graph half of `preprocess(graph)` — run.py:133-148.  `reorder` ("degree" | "community", default None): renumber
    the vertices for locality afterwards (see `reorder_graph`); results of the stacks are unchanged and stay in original order."""
    feat = g.ndata.get("feat")
    g = to_bidirected(g)
    if feat is not None:
        g.ndata["feat"] = feat
    g = g.remove_self_loop().add_self_loop()
    if reorder:
        g = reorder_graph(g, reorder, plan_order)
    g.create_formats_()
    return g
