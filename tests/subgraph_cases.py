"""Induced-subgraph extraction restated in numpy (the contract of bot_subgraph_*_i32, include/bot_gnn.h), shared by
tests/test_subgraph_host.py (where it is itself checked against a dense adjacency and scipy.sparse, and stands in for the kernels
on CPU graphs) and tests/test_subgraph_gpu.py (which holds the kernels to it bit for bit)."""
import numpy as np
import torch

# constants of csrc/subgraph.hip the GPU cases are sized against
LONG_ROW = 2048          # kSubLongRow: longer rows are swept by a 1024-thread workgroup
LONG_TILE = 4096         # kSubLongTile: positions per step of that sweep


def induced_reference(indptr, indices, eid, nodes):
    """(offsets int64 [n + 1], local_src int32 [E_sub], parent_eid int32 [E_sub]): row i = the in-edges of nodes[i] (CSC row of the
    parent) whose source is in `nodes`, in the parent's CSC position order; local id = position in `nodes` (unique ids)."""
    indptr, indices, eid, nodes = (np.asarray(a, dtype=np.int64) for a in (indptr, indices, eid, nodes))
    n = len(nodes)
    local = np.full(len(indptr) - 1, -1, dtype=np.int64)
    local[nodes] = np.arange(n)
    deg = indptr[nodes + 1] - indptr[nodes]
    row = np.repeat(np.arange(n), deg)
    first = np.cumsum(deg) - deg                                     # where row i starts in the list of scanned positions
    pos = np.repeat(indptr[nodes] - first, deg) + np.arange(int(deg.sum()))
    src = local[indices[pos]]
    keep = src >= 0
    offsets = np.zeros(n + 1, dtype=np.int64)
    offsets[1:] = np.cumsum(np.bincount(row[keep], minlength=n))
    return offsets, src[keep].astype(np.int32), eid[pos[keep]].astype(np.int32)


def csc_arrays(g):
    c = g.csc
    return c.indptr.cpu().numpy(), c.indices.cpu().numpy(), c.eid.cpu().numpy()


def node_subgraph_standin(csc, nodes, node_map):
    """bot_amd._C.node_subgraph on CPU tensors: the restatement, with the wrapper's errors (the map is never touched)."""
    ids = nodes.cpu().numpy().astype(np.int64)
    n_nodes = int(node_map.numel())
    if len(ids) and (ids.min() < 0 or ids.max() >= n_nodes or len(np.unique(ids)) != len(ids)):
        raise ValueError("node_subgraph: duplicate or out-of-range ids")
    off, src, pe = induced_reference(csc.indptr.cpu().numpy(), csc.indices.cpu().numpy(), csc.eid.cpu().numpy(), ids)
    dev = nodes.device
    return torch.from_numpy(off).to(dev), torch.from_numpy(src).to(dev), torch.from_numpy(pe).to(dev)


def dense_adjacency(g):
    """A[dst, src] = edge id + 1 (0: no edge) of a graph without parallel edges."""
    s, d = (t.cpu().numpy() for t in g.edges())
    n = g.number_of_nodes()
    A = np.zeros((n, n), dtype=np.int64)
    assert len(np.unique(d * n + s)) == len(s), "dense_adjacency takes a graph without parallel edges"
    A[d, s] = np.arange(len(s)) + 1
    return A


def dense_of_subgraph(n, offsets, local_src, parent_eid):
    B = np.zeros((n, n), dtype=np.int64)
    rows = np.repeat(np.arange(n), np.diff(offsets))
    B[rows, local_src] = parent_eid.astype(np.int64) + 1
    return B
