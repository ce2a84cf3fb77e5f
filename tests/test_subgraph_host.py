"""Induced-subgraph (cluster) batches without a GPU: the numpy restatement of the extraction contract (tests/subgraph_cases.py)
against a dense adjacency and scipy.sparse, the exported symbols and their argument checks, `cluster_assignment`, `ClusterLoader`
and the `Subgraph` object on CPU graphs.  tests/test_subgraph_gpu.py holds the kernels to the restatement bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import bot_amd
from bot_amd import synth
from bot_amd.graph import reorder_graph
from tests import subgraph_cases as SC


def _graph(n=300, e_raw=2500, seed=1, loops=True):
    rs, rd = synth.powerlaw_edges(n, e_raw, seed)
    g = bot_amd.to_bidirected(bot_amd.Graph(rs, rd, n)).remove_self_loop()      # no parallel edges
    return g.add_self_loop() if loops else g


def _node_sets(n, seed=0):
    rng = np.random.default_rng(seed)
    return [np.zeros(0, dtype=np.int64), np.array([n // 2]), np.arange(n), rng.permutation(n), rng.permutation(n)[:n // 7],
            np.sort(rng.permutation(n)[:n // 3])]


@pytest.mark.parametrize("loops", [True, False])
def test_restatement_against_a_dense_adjacency(loops):
    g = _graph(loops=loops)
    indptr, indices, eid = SC.csc_arrays(g)
    A = SC.dense_adjacency(g)
    for nodes in _node_sets(g.number_of_nodes()):
        off, src, pe = SC.induced_reference(indptr, indices, eid, nodes)
        assert off[0] == 0 and off[-1] == len(src) == len(pe) and np.all(np.diff(off) >= 0)
        want = A[np.ix_(nodes, nodes)]
        assert np.array_equal(SC.dense_of_subgraph(len(nodes), off, src, pe), want)
        assert len(src) == int((want > 0).sum())                                  # no entry written twice
        for i in range(len(nodes)):                                               # parent CSC position order inside a row: ascending
            assert np.all(np.diff(pe[off[i]:off[i + 1]]) > 0)                     # edge id (the parent's CSC is stable in it)
    if not loops:
        nodes = _node_sets(g.number_of_nodes())[4]
        assert np.any(np.diff(SC.induced_reference(indptr, indices, eid, nodes)[0]) == 0)     # some row keeps nothing
    off, src, pe = SC.induced_reference(indptr, indices, eid, np.arange(g.number_of_nodes()))
    assert np.array_equal(off, indptr) and np.array_equal(src, indices) and np.array_equal(pe, eid)    # identity: the parent's CSC


def test_restatement_against_scipy_sparse():
    sp = pytest.importorskip("scipy.sparse")
    g = _graph(n=500, e_raw=6000, seed=4)
    indptr, indices, eid = SC.csc_arrays(g)
    n = g.number_of_nodes()
    M = sp.csr_matrix((eid.astype(np.int64) + 1, indices, indptr), shape=(n, n))      # rows = destinations
    for nodes in _node_sets(n, seed=3)[1:]:
        off, src, pe = SC.induced_reference(indptr, indices, eid, nodes)
        want = M[nodes][:, nodes].toarray()
        assert np.array_equal(SC.dense_of_subgraph(len(nodes), off, src, pe), want)


def test_subgraph_symbols_are_exported_and_validate_arguments():
    from bot_amd import _C
    lib = _C._lib
    for name in ("bot_subgraph_mark_i32", "bot_subgraph_count_i32", "bot_subgraph_fill_i32", "bot_subgraph_unmark_i32"):
        assert name in _C.EXPORTED and hasattr(lib, name)
    assert lib.bot_abi_version() == 19
    buf = (ctypes.c_int32 * 16)()
    off = (ctypes.c_int64 * 16)()
    p, o = ctypes.addressof(buf), ctypes.addressof(off)
    # NULL pointers -> BOT_E_NULL
    assert lib.bot_subgraph_mark_i32(None, 2, p, 4, o, None) == -1
    assert lib.bot_subgraph_mark_i32(p, 2, None, 4, o, None) == -1
    assert lib.bot_subgraph_mark_i32(p, 2, p, 4, None, None) == -1
    assert lib.bot_subgraph_count_i32(None, p, 4, p, 2, p, p, None) == -1
    assert lib.bot_subgraph_count_i32(p, p, 4, p, 2, None, p, None) == -1
    assert lib.bot_subgraph_count_i32(p, p, 4, p, 2, p, None, None) == -1
    assert lib.bot_subgraph_fill_i32(p, p, None, 4, p, 2, p, o, p, p, None) == -1
    assert lib.bot_subgraph_fill_i32(p, p, p, 4, p, 2, p, None, p, p, None) == -1
    assert lib.bot_subgraph_fill_i32(p, p, p, 4, p, 2, p, o, None, p, None) == -1
    assert lib.bot_subgraph_unmark_i32(None, 2, p, 4, None) == -1
    assert lib.bot_subgraph_unmark_i32(p, 2, None, 4, None) == -1
    # negative sizes, more nodes than the graph has -> BOT_E_RANGE
    assert lib.bot_subgraph_mark_i32(p, -1, p, 4, o, None) == -2
    assert lib.bot_subgraph_mark_i32(p, 2, p, -4, o, None) == -2
    assert lib.bot_subgraph_mark_i32(p, 5, p, 4, o, None) == -2
    assert lib.bot_subgraph_count_i32(p, p, -4, p, 2, p, p, None) == -2
    assert lib.bot_subgraph_count_i32(p, p, 4, p, 5, p, p, None) == -2
    assert lib.bot_subgraph_fill_i32(p, p, p, 4, p, -2, p, o, p, p, None) == -2
    assert lib.bot_subgraph_fill_i32(p, p, p, 4, p, 5, p, o, p, p, None) == -2
    assert lib.bot_subgraph_unmark_i32(p, 5, p, 4, None) == -2
    assert lib.bot_subgraph_unmark_i32(p, -1, p, 4, None) == -2
    assert b"subgraph_unmark" in lib.bot_last_error()
    # an empty node set is a no-op: nothing launched, so no GPU is needed
    assert lib.bot_subgraph_mark_i32(None, 0, p, 4, o, None) == 0
    assert lib.bot_subgraph_count_i32(p, None, 4, None, 0, p, None, None) == 0
    assert lib.bot_subgraph_fill_i32(p, None, None, 4, None, 0, p, None, None, None, None) == 0
    assert lib.bot_subgraph_unmark_i32(None, 0, p, 4, None) == 0


def test_cluster_assignment_covers_balances_and_is_seeded():
    from bot_amd.sampling import cluster_assignment
    g = _graph(n=1003, e_raw=9000, seed=2)
    for method in ("community", "random"):
        for n_parts in (1, 7, 30):
            parts = cluster_assignment(g, n_parts, method, seed=5)
            assert parts.dtype == torch.int32 and parts.shape == (1003,)                  # every node in exactly one part
            sizes = torch.bincount(parts.long(), minlength=n_parts)
            assert sizes.numel() == n_parts and int(parts.min()) == 0
            assert int(sizes.max()) - int(sizes.min()) <= 1 and int(sizes.sum()) == 1003
            assert torch.equal(parts, cluster_assignment(g, n_parts, method, seed=5))
    assert not torch.equal(cluster_assignment(g, 7, "random", seed=5), cluster_assignment(g, 7, "random", seed=6))
    with pytest.raises(ValueError):
        cluster_assignment(g, 7, "metis")
    with pytest.raises(ValueError):
        cluster_assignment(g, 0)
    with pytest.raises(ValueError):
        cluster_assignment(g, 2000)


def test_community_parts_keep_more_edges_than_random_parts():
    """Planted graph: synth.community_edges(6000, 60000, seed 3, n_blocks=8, p_in=0.9), preprocessed; 8 parts.  Share of the
    non-loop edges with both ends in one part, measured on the CPU: 0.907 under "community", 0.128 under "random" (expectation
    1 / 8 = 0.125).  The assertion is the ordering; the random share is also held to its expectation (within 0.02, several
    standard deviations of a share taken over some 10^5 edges, the hubs' correlated edges included; seeded, so deterministic)."""
    from bot_amd.sampling import cluster_assignment
    n, n_parts = 6000, 8
    s, d = synth.community_edges(n, 60000, 3, n_blocks=8, p_in=0.9)
    g = bot_amd.preprocess(bot_amd.Graph(s, d, n))
    gs, gd = g.edges()
    keep = gs != gd
    share = {}
    for method in ("community", "random"):
        parts = cluster_assignment(g, n_parts, method, seed=0).long()
        share[method] = float((parts[gs[keep]] == parts[gd[keep]]).float().mean())
    print(share)
    assert share["community"] > share["random"]
    assert abs(share["random"] - 1.0 / n_parts) < 0.02


@pytest.fixture
def standin(monkeypatch):
    from bot_amd import _C
    monkeypatch.setattr(_C, "node_subgraph", SC.node_subgraph_standin)


def test_cluster_loader_covers_every_node_once_per_epoch(standin):
    from bot_amd.sampling import ClusterLoader, Subgraph, cluster_assignment
    g = _graph(n=700, e_raw=5000, seed=3)
    n = g.number_of_nodes()
    parts = cluster_assignment(g, 9, "random", seed=1)
    for ppb in (1, 2, 4):
        loader = ClusterLoader(g, parts, parts_per_batch=ppb, seed=3)
        assert len(loader) == -(-9 // ppb)
        for _ in range(2):
            seen, batches = [], 0
            for sub in loader:
                assert isinstance(sub, Subgraph) and not sub.is_block and sub.halo is None and sub.node_perm is None
                ids = sub.parent_nid.long()
                assert torch.all(ids[1:] > ids[:-1])                                       # ascending parent id inside the batch
                assert len(torch.unique(parts[ids])) <= ppb
                seen.append(ids)
                batches += 1
            assert batches == len(loader)
            assert torch.equal(torch.sort(torch.cat(seen)).values, torch.arange(n))        # every node exactly once
    # the same seed gives the same batches; another seed another order
    a = [b.clone() for b in ClusterLoader(g, parts, 2, seed=3).node_batches()]
    b = [b.clone() for b in ClusterLoader(g, parts, 2, seed=3).node_batches()]
    c = [b.clone() for b in ClusterLoader(g, parts, 2, seed=4).node_batches()]
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and not all(torch.equal(x, y) for x, y in zip(a, c))
    # every part in one batch: one batch, the whole graph, its CSC the parent's
    loader = ClusterLoader(g, parts, parts_per_batch=9, seed=0)
    subs = list(loader)
    assert len(loader) == 1 and len(subs) == 1
    sub = subs[0]
    assert torch.equal(sub.parent_nid.long(), torch.arange(n)) and sub.number_of_edges() == g.number_of_edges()
    assert torch.equal(sub.csc.indptr, g.csc.indptr) and torch.equal(sub.csc.indices, g.csc.indices)
    assert torch.equal(sub.parent_eid, g.csc.eid)
    with pytest.raises(ValueError):
        ClusterLoader(g, parts[:-1])
    with pytest.raises(ValueError):
        ClusterLoader(g, parts, parts_per_batch=0)


@pytest.mark.parametrize("reordered", [False, True])
def test_subgraph_object_from_host_built_arrays(reordered):
    from bot_amd.sampling import Subgraph
    g = _graph(n=400, e_raw=3000, seed=6)
    n, E = g.number_of_nodes(), g.number_of_edges()
    gen = torch.Generator().manual_seed(1)
    g.ndata["feat"] = torch.randn(n, 5, generator=gen)
    g.edata["w"] = torch.randn(E, 2, generator=gen)
    if reordered:
        g = reorder_graph(g, "degree")
    nodes = torch.randperm(n, generator=gen)[:150]
    off, src, pe = SC.induced_reference(*SC.csc_arrays(g), nodes.numpy())
    sub = Subgraph(g, nodes.to(torch.int32), torch.from_numpy(off), torch.from_numpy(src), torch.from_numpy(pe))
    assert sub.number_of_nodes() == sub.number_of_src_nodes() == sub.number_of_dst_nodes() == 150
    assert not sub.is_block and sub.halo is None and sub.node_perm is None and sub.number_of_edges() == len(src)
    assert torch.equal(sub.parent_nid.long(), nodes) and torch.equal(sub.parent_eid.long(), torch.from_numpy(pe).long())
    # the edge list is the induced one: edge e of the subgraph is parent edge parent_eid[e] between the same (relabelled) nodes
    ps, pd = g.edges()
    s, d = sub.edges()
    assert torch.equal(nodes[s], ps[sub.parent_eid.long()]) and torch.equal(nodes[d], pd[sub.parent_eid.long()])
    inside = torch.zeros(n, dtype=torch.bool)
    inside[nodes] = True
    assert sub.number_of_edges() == int((inside[ps] & inside[pd]).sum())
    # its own degrees, not the parent's
    indeg = (sub.csc.indptr[1:] - sub.csc.indptr[:-1]).long()
    assert torch.equal(indeg, torch.bincount(d, minlength=150)) and int(indeg.min()) >= 1       # every row keeps its self-loop
    outdeg = (sub.csr.indptr[1:] - sub.csr.indptr[:-1]).long()
    assert torch.equal(outdeg, torch.bincount(s, minlength=150))
    parent_in = (g.csc.indptr[1:] - g.csc.indptr[:-1]).long()
    assert torch.all(indeg <= parent_in[nodes]) and int((indeg < parent_in[nodes]).sum()) > 0
    assert torch.equal(sub.csc.eid.long(), torch.arange(len(src)))                                # edge id = CSC position
    # lazy gathers, through node_perm when the parent was reordered (its frames stay in original order)
    assert not dict.__contains__(sub.ndata, "feat") and "feat" in sub.ndata and "w" in sub.edata
    rows = nodes if not reordered else g.node_perm[nodes]
    assert torch.equal(sub.parent_rows, rows)
    assert torch.equal(sub.ndata["feat"], g.ndata["feat"][rows]) and dict.__contains__(sub.ndata, "feat")
    assert torch.equal(sub.edata["w"], g.edata["w"][sub.parent_eid.long()])
    sub.ndata["feat"] = torch.zeros(150, 1)                                                        # writes stay local
    assert g.ndata["feat"].shape == (n, 5)
    with pytest.raises(ValueError):
        Subgraph(g, nodes.to(torch.int32), torch.from_numpy(off)[:-1], torch.from_numpy(src), torch.from_numpy(pe))


def test_block_and_subgraph_share_one_constructor():
    """A `Block` and a `Subgraph` built from the same CSC arrays (6 rows of 9, 0, 1, 0, 2, 0 edges under chunk = 4: one row longer
    than the chunk, a short row, empty rows) carry the same CSC direction and row plan; only what they are differs."""
    from bot_amd.sampling import Block, Subgraph
    parent = bot_amd.Graph(torch.arange(12) % 6, torch.arange(12) // 2, 6, chunk=4)
    ids = torch.arange(6, dtype=torch.int32)
    offsets = torch.tensor([0, 9, 9, 10, 10, 12, 12])
    local_src = torch.tensor([0, 1, 2, 3, 4, 5, 0, 1, 2, 3, 4, 5], dtype=torch.int32)
    parent_eid = torch.arange(12, dtype=torch.int32)
    block = Block(parent, ids, offsets, local_src, parent_eid)
    sub = Subgraph(parent, ids, offsets, local_src, parent_eid)
    a, b = block.csc, sub.csc
    for name in ("indptr", "indices", "eid", "items", "long_rows", "long_ptr"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    for name in ("n_rows", "nnz", "n_items", "n_long", "n_slots", "chunk"):
        assert getattr(a, name) == getattr(b, name), name
    assert a.n_long == 1 and a.chunk == 4 and a.n_rows == 6 and a.nnz == 12
    # the plan itself, {row, begin, end, slot}: row 0 in three chunks with slots 0..2, then the short rows longest first, then the empty ones
    assert a.items.tolist() == [[0, 0, 4, 0], [0, 4, 8, 1], [0, 8, 9, 2], [4, 10, 12, -1], [2, 9, 10, -1], [1, 9, 9, -1], [3, 10, 10, -1],
                                [5, 12, 12, -1]]
    assert a.long_rows.tolist() == [0] and a.long_ptr.tolist() == [0, 3] and a.n_items == 8 and a.n_slots == 3
    assert torch.equal(a.indptr.long(), offsets) and torch.equal(a.indices, local_src)
    assert torch.equal(block.src32, sub.src32) and torch.equal(block.dst32, sub.dst32)
    assert torch.equal(block.src32, local_src) and block.dst32.tolist() == [0] * 9 + [2] + [4, 4]
    assert block.is_block and block.number_of_dst_nodes() == 6 and block.number_of_src_nodes() == 6
    assert not sub.is_block and sub.number_of_nodes() == 6
    assert torch.equal(block.parent_eid, sub.parent_eid) and torch.equal(block.src_nid, sub.parent_nid)


def test_graph_subgraph_refuses_what_it_cannot_serve(standin):
    g = _graph(n=200, e_raw=1500, seed=7)
    sub = g.subgraph([5, 3, 9])                                                                    # the DGL name, host ids
    assert sub.number_of_nodes() == 3 and sub.parent_nid.tolist() == [5, 3, 9]
    with pytest.raises(ValueError, match="unique"):
        g.subgraph([1, 2, 1])
    with pytest.raises(ValueError, match="out of range"):
        g.subgraph(torch.tensor([0, 200]))
    with pytest.raises(ValueError, match="out of range"):
        g.subgraph(torch.tensor([-1, 3]))
    with pytest.raises(ValueError):
        g.subgraph(torch.tensor([0.5, 1.0]))
    with pytest.raises(ValueError):
        g.subgraph(torch.tensor([[0, 1]]))
    s, d = g.edges()
    keep = d < 100
    block = bot_amd.Graph(s[keep], d[keep], 200, num_dst_nodes=100)
    with pytest.raises(ValueError, match="whole graph"):
        block.subgraph([1, 2])
    part = _graph(n=200, e_raw=1500, seed=7)
    part.halo = object()                                                                           # a partition's block carries a halo plan
    with pytest.raises(ValueError, match="whole graph"):
        part.subgraph([1, 2])
    with pytest.raises(NotImplementedError):
        sub.to("meta")
    assert sub.to("cpu") is sub


def test_build_clustered_names_and_defaults():
    from bot_amd import workloads
    assert workloads.CLUSTERED == {"arxiv": 30, "reddit": 30, "cora": 5, "products": 30, "proteins": 10}
    with pytest.raises(ValueError):
        workloads.build_clustered("citeseer", "cpu")
    from bot_amd import minibatch
    with pytest.raises(ValueError):
        minibatch.train_epoch_subgraphs(None, None, None, None, None)
    roles = minibatch.node_roles(6, torch.tensor([0, 2]), torch.tensor([3]), torch.tensor([5]))
    assert roles.tolist() == [1, 0, 1, 2, 0, 3]
