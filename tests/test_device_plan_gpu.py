"""The device graph builder (csrc/plan.hip) on the MI355X, held bit for bit to the host path it replaces: the row planner against
`_C.row_plan` on the same offsets, the CSC transpose against `graph.build_direction` on the same edges, two calls against each other,
and the mini-batch graphs of S-arxiv (sampled blocks, an induced subgraph, a GraphSAINT batch, a cluster batch) built under both
settings of `graph.DEVICE_PLAN`, with one train step of a GAT on a subgraph and of a GCN on a block list under each."""
import importlib

import pytest
import torch
import torch.nn.functional as F

import bot_amd
from bot_amd import _C, synth
from bot_amd import nn as bnn
from bot_amd.sampling import ClusterLoader, MultiLayerNeighborSampler, SAINTSampler, cluster_assignment, node_subgraph

G = importlib.import_module("bot_amd.graph")            # (bot_amd.graph the attribute is dgl.graph's stand-in, a function)

pytestmark = pytest.mark.gpu
DEV = "cuda"
FIELDS = ("indptr", "indices", "eid", "items", "long_rows", "long_ptr", "n_rows", "nnz", "n_items", "n_long", "n_slots", "chunk", "plan_order")


def _same(a, b, what):
    if a is None or b is None:
        assert a is None and b is None, what
    elif isinstance(a, torch.Tensor):
        assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.cpu(), b.cpu()), what
    else:
        assert a == b, (what, a, b)


def _indptr(deg):
    out = torch.zeros(len(deg) + 1, dtype=torch.int64)
    out[1:] = torch.cumsum(torch.as_tensor(deg, dtype=torch.int64), 0)
    assert int(out[-1]) < 2 ** 31 - 1
    return out.to(torch.int32)


def _check_plan(indptr, chunk):
    """Every array and every size of the device plan equals the host planner's on the same offsets."""
    want = _C.row_plan(indptr.contiguous(), chunk)
    c0 = _C.PLAN_COUNTS["device_plan"]
    got = _C.row_plan_device(indptr.to(DEV), chunk)
    assert _C.PLAN_COUNTS["device_plan"] == c0 + 1
    for a, b, what in zip(got, want, ("items", "long_rows", "long_ptr", "n_slots")):
        assert not isinstance(a, torch.Tensor) or a.is_cuda
        _same(a, b, f"{what} (chunk {chunk}, {indptr.numel() - 1} rows)")
    return got


def _degree_families(n_rows, chunk):
    gen = torch.Generator().manual_seed(1000 * chunk + n_rows)
    short = lambda: torch.randint(0, min(chunk, 8) + 1, (n_rows,), generator=gen)
    yield "zeros", torch.zeros(n_rows, dtype=torch.int64)
    edge = torch.tensor([chunk, chunk + 1, 2 * chunk, 2 * chunk + 1])
    yield "at the chunk", edge[torch.arange(n_rows) % 4]
    yield "at the chunk, shuffled", edge[torch.randint(0, 4, (n_rows,), generator=gen)]
    hub = short()
    hub[n_rows // 2] = 5000
    yield "one hub", hub
    hubs = short()
    for i, d in enumerate((5000, 2100, 3 * chunk + 1, chunk + 1, 2049)):
        hubs[min(n_rows // 3 + i, n_rows - 1)] = d
    yield "hubs in a row", hubs


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 4097])
@pytest.mark.parametrize("chunk", [1, 4, 64, 512])
def test_planner_against_the_host_planner(chunk, n_rows):
    for name, deg in _degree_families(n_rows, chunk):
        items, long_rows, long_ptr, n_slots = _check_plan(_indptr(deg), chunk)
        if name == "zeros":
            assert long_rows.numel() == 0 and n_slots == 0 and items.shape[0] == n_rows
        if name == "one hub" and chunk < 5000:
            assert long_rows.numel() >= 1 and n_slots >= -(-5000 // chunk)


@pytest.fixture(scope="module")
def powerlaw():
    """synth.powerlaw_edges(20000, 137000, s) after preprocessing, on the host: (graph, CSC offsets, CSC sources)."""
    out = []
    for s in (3, 4):
        rs, rd = synth.powerlaw_edges(20000, 137000, s)
        g = bot_amd.preprocess(bot_amd.Graph(rs, rd, 20000))
        out.append((g, g.csc.indptr.clone(), g.csc.indices.clone()))
    return out


@pytest.mark.parametrize("chunk", [1, 4, 64, 512])
def test_planner_on_a_power_law_graph(powerlaw, chunk):
    for g, indptr, _ in powerlaw:
        _check_plan(indptr, chunk)
    _check_plan(powerlaw[0][0].csr.indptr, chunk)


def test_a_non_monotone_indptr_raises_and_the_next_call_is_correct():
    bad = torch.tensor([0, 5, 3, 8, 8, 200], dtype=torch.int32)
    with pytest.raises(_C.BotKernelError, match="rc=-4"):                       # the host planner's BOT_E_PLAN
        _C.row_plan_device(bad.to(DEV), 4)
    with pytest.raises(_C.BotKernelError, match="rc=-4"):
        _C.row_plan(bad, 4)
    _check_plan(torch.tensor([0, 5, 5, 8, 8, 200], dtype=torch.int32), 4)


def test_a_chunk_above_the_device_bound_goes_to_the_host_planner(powerlaw):
    indptr = powerlaw[0][1]
    c0 = dict(_C.PLAN_COUNTS)
    got = _C.row_plan_device(indptr.to(DEV), 2000)
    assert _C.PLAN_COUNTS["host_plan"] == c0["host_plan"] + 1 and _C.PLAN_COUNTS["device_plan"] == c0["device_plan"]
    for a, b in zip(got, _C.row_plan(indptr, 2000)):
        _same(a, b, "chunk 2000")


def _check_transpose(indptr, indices, n_src):
    """indptr_r / indices_r / eid_r equal `build_direction` on the CPU copy of the same edges; eid_r is csr2csc computed the old way."""
    n_dst, E = indptr.numel() - 1, indices.numel()
    dst = torch.repeat_interleave(torch.arange(n_dst), (indptr[1:] - indptr[:-1]).long())
    want = G.build_direction(indices.long(), dst, n_src)
    c0 = _C.PLAN_COUNTS["device_transpose"]
    got = _C.csc_transpose(indptr.to(DEV), indices.to(DEV).contiguous(), n_src)
    assert _C.PLAN_COUNTS["device_transpose"] == c0 + 1
    for a, b, what in zip(got, (want.indptr, want.indices, want.eid), ("indptr", "indices", "eid")):
        assert a.is_cuda
        _same(a, b, f"{what} (n_src {n_src}, n_dst {n_dst}, E {E})")
    csc_eid = torch.arange(E, dtype=torch.int32)                                # a batch graph's edge id is its CSC position
    inverse = torch.empty_like(csc_eid)
    inverse[csc_eid.long()] = torch.arange(E, dtype=torch.int32)
    _same(got[2], G.take_rows(inverse, want.eid).contiguous(), "csr2csc")       # Graph.csr2csc's formula
    return got


def _random_csc(n_dst, n_src, E, seed, lo=0, hi=None):
    """E entries over n_dst rows (some of them empty), sources drawn from [lo, hi)."""
    gen = torch.Generator().manual_seed(seed)
    hi = n_src if hi is None else hi
    dst = torch.sort(torch.randint(0, n_dst, (E,), generator=gen)).values if n_dst else torch.zeros(0, dtype=torch.int64)
    indptr = torch.zeros(n_dst + 1, dtype=torch.int64)
    indptr[1:] = torch.cumsum(torch.bincount(dst, minlength=n_dst), 0)
    src = torch.randint(lo, hi, (E,), generator=gen) if E else torch.zeros(0, dtype=torch.int64)
    return indptr.to(torch.int32), src.to(torch.int32)


TRANSPOSE_CASES = {     # name: (n_dst, n_src, E, lo, hi)
    "no entries": (7, 9, 0, 0, None),
    "no rows": (0, 0, 0, 0, None),
    "one source": (50, 1, 300, 0, None),                     # every edge parallel to others; one radix pass
    "64 sources": (64, 64, 1000, 0, None),
    "65 sources, square": (65, 65, 4097, 0, None),           # one entry beyond a sort tile
    "block": (700, 3000, 9000, 0, None),                     # n_src > n_dst; two passes
    "empty sources in front and behind": (500, 2000, 6000, 300, 1500),
    "parallel edges": (40, 20000, 5000, 100, 104),           # four sources: the same (src, dst) pair many times
    "20000 sources": (20000, 20000, 157000, 0, None),
    "three passes": (300, 70000, 5000, 0, None),
    "four passes": (300, 2 ** 24 + 5, 5000, 2 ** 24 - 300, None),
}


@pytest.mark.parametrize("case", list(TRANSPOSE_CASES))
def test_transpose_against_build_direction(case):
    n_dst, n_src, E, lo, hi = TRANSPOSE_CASES[case]
    indptr, indices = _random_csc(n_dst, n_src, E, 11, lo, hi)
    indptr_r, indices_r, eid_r = _check_transpose(indptr, indices, n_src)
    if case == "parallel edges":
        dst =torch.repeat_interleave(torch.arange(n_dst), (indptr[1:] - indptr[:-1]).long())
        keys = indices.long() * n_dst + dst
        assert int(torch.unique(keys).numel()) < E // 4                          # the same pair several times
        deg = (indptr_r[1:] - indptr_r[:-1]).cpu()
        assert int((deg > 0).sum()) == 4 and bool((deg[:100] == 0).all()) and bool((deg[104:] == 0).all())


def test_transpose_with_a_hub_source(powerlaw):
    """A source with more than 2 048 out-edges: one in every row of a block, next to random ones; and the power-law graph's own hubs."""
    n_dst, n_src = 3000, 5000
    gen = torch.Generator().manual_seed(5)
    extra = torch.randint(0, 4, (n_dst,), generator=gen)
    indptr = _indptr(extra + 1)
    indices = torch.randint(0, n_src, (int(indptr[-1]),), generator=gen).to(torch.int32)
    indices[indptr[:-1].long() + torch.div(extra, 2, rounding_mode="floor")] = 77          # somewhere inside each row
    indptr_r, _, _ = _check_transpose(indptr, indices, n_src)
    assert int(indptr_r[78] - indptr_r[77]) >= 3000 > 2048
    g, indptr, indices = powerlaw[0]
    indptr_r, _, _ = _check_transpose(indptr, indices, 20000)
    _same(indptr_r, g.csr.indptr, "the graph's own CSR offsets")


def test_an_index_out_of_range_raises():
    indptr, indices = _random_csc(50, 80, 400, 2)
    for value in (80, -1, 2 ** 31 - 1):
        bad = indices.clone()
        bad[123] = value
        with pytest.raises(_C.BotKernelError, match="outside"):
            _C.csc_transpose(indptr.to(DEV), bad.to(DEV), 80)
    _check_transpose(indptr, indices, 80)


def test_two_calls_give_the_same_bytes(powerlaw):
    _, indptr, indices = powerlaw[1]
    a, b = indptr.to(DEV), indices.to(DEV)
    raw = lambda ts: [t.cpu().numpy().tobytes() if isinstance(t, torch.Tensor) else t for t in ts]
    assert raw(_C.row_plan_device(a, 4)) == raw(_C.row_plan_device(a, 4))
    assert raw(_C.row_plan_device(a, 64)) == raw(_C.row_plan_device(a, 64))
    assert raw(_C.csc_transpose(a, b, 20000)) == raw(_C.csc_transpose(a, b, 20000))


# ------------------------------------------------------------------------------------------------ end to end on S-arxiv
@pytest.fixture(scope="module")
def arxiv():
    from bot_amd import workloads
    wl = workloads.build("arxiv", DEV, scale=0.05, seed=0, drop=False)
    wl.graph.ndata["feat"] = wl.dataset.feat
    return wl


def _batch_graphs(wl):
    g, ds = wl.graph, wl.dataset
    n = g.number_of_nodes()
    blocks = MultiLayerNeighborSampler([10, 10, 10]).sample_blocks(g, ds.train_idx[:400], torch.Generator().manual_seed(3))
    nodes = torch.randperm(n, generator=torch.Generator().manual_seed(2))[:n // 3].to(DEV)
    loader = ClusterLoader(g, cluster_assignment(g, 30, "random", seed=1), parts_per_batch=2, seed=0)
    graphs = blocks + [node_subgraph(g, nodes), SAINTSampler("walk", (n // 30, 2)).sample(g, 12345), next(iter(loader))]
    for b in graphs:
        _ = b.csc, b.csr, b.csr2csc
    return graphs


def test_batch_graphs_are_equal_under_both_settings(arxiv, monkeypatch):
    monkeypatch.delenv("BOT_DEVICE_PLAN", raising=False)
    monkeypatch.setattr(G, "DEVICE_PLAN", True)
    c0 = dict(_C.PLAN_COUNTS)
    on_device = _batch_graphs(arxiv)
    c1 = dict(_C.PLAN_COUNTS)
    k = len(on_device)
    assert k == 6
    assert c1["device_plan"] - c0["device_plan"] == 2 * k and c1["device_transpose"] - c0["device_transpose"] == k
    assert c1["host_plan"] == c0["host_plan"]
    monkeypatch.setattr(G, "DEVICE_PLAN", False)
    on_host = _batch_graphs(arxiv)
    c2 = dict(_C.PLAN_COUNTS)
    assert c2["device_plan"] == c1["device_plan"] and c2["device_transpose"] == c1["device_transpose"]
    assert c2["host_plan"] - c1["host_plan"] == 2 * k
    monkeypatch.setattr(G, "DEVICE_PLAN", True)
    monkeypatch.setenv("BOT_DEVICE_PLAN", "0")                                   # the environment switch, read at call time
    _batch_graphs(arxiv)
    assert _C.PLAN_COUNTS["device_plan"] == c2["device_plan"] and _C.PLAN_COUNTS["host_plan"] - c2["host_plan"] == 2 * k
    for i, (a, b) in enumerate(zip(on_device, on_host)):
        assert type(a) is type(b) and a.number_of_src_nodes() == b.number_of_src_nodes()
        for side in ("csc", "csr"):
            da, db = getattr(a, side), getattr(b, side)
            for f in FIELDS:
                _same(getattr(da, f), getattr(db, f), f"graph {i} {side}.{f}")
            assert da.indptr.is_cuda and da.items.is_cuda
        _same(a.csr2csc, b.csr2csc, f"graph {i} csr2csc")


def _train_step(model, run, labels):
    model.train()
    model.zero_grad(set_to_none=True)
    logits = run()
    loss = F.cross_entropy(logits, labels)
    loss.backward()
    return [loss.detach().clone(), logits.detach().clone()] + [p.grad.detach().clone() for p in model.parameters()]


def _bit_identical(on_device, on_host, model):
    names = ["loss", "logits"] + [k for k, _ in model.named_parameters()]
    assert len(on_device) == len(on_host) == len(names)
    for name, a, b in zip(names, on_device, on_host):
        assert torch.equal(a, b), (name, float((a - b).abs().max()))


def test_gat_step_on_a_subgraph_is_bit_identical_under_both_settings(arxiv, monkeypatch):
    monkeypatch.delenv("BOT_DEVICE_PLAN", raising=False)
    g, ds = arxiv.graph, arxiv.dataset
    n, C = g.number_of_nodes(), ds.n_classes
    nodes = torch.randperm(n, generator=torch.Generator().manual_seed(6))[:n // 3].to(DEV)
    torch.manual_seed(0)
    model = bnn.GAT(dim_node=ds.feat.shape[1], dim_edge=0, dim_output=C, activation=F.relu, n_layers=3, n_heads=3, n_hidden=32, norm="batch",
                    non_interactive_attn=True, use_symmetric_norm=False, linear=True, residual=False, dropout=0.0, input_drop=0.0,
                    attn_drop=0.0, edge_drop=0.0).to(DEV)
    out = []
    for flag in (True, False):
        monkeypatch.setattr(G, "DEVICE_PLAN", flag)
        c0 = dict(_C.PLAN_COUNTS)
        torch.manual_seed(1)
        sub = node_subgraph(g, nodes)
        labels = ds.labels[sub.parent_rows, 0]
        out.append(_train_step(model, lambda: model(sub, sub.ndata["feat"]), labels))
        assert (_C.PLAN_COUNTS["device_plan"] - c0["device_plan"] == 2) == flag         # the CSC's plan and, at the backward, the CSR's
        assert (_C.PLAN_COUNTS["host_plan"] - c0["host_plan"] == 2) == (not flag)
    _bit_identical(out[0], out[1], model)


def test_gcn_step_on_a_block_list_is_bit_identical_under_both_settings(arxiv, monkeypatch):
    monkeypatch.delenv("BOT_DEVICE_PLAN", raising=False)
    g, ds = arxiv.graph, arxiv.dataset
    torch.manual_seed(0)
    model = bnn.GCN(in_feats=ds.feat.shape[1], n_classes=ds.n_classes, n_hidden=32, n_layers=3, activation=F.relu, norm="batch",
                    norm_adj="symm", dropout=0.0, use_linear=True).to(DEV)
    out = []
    for flag in (True, False):
        monkeypatch.setattr(G, "DEVICE_PLAN", flag)
        c0 = dict(_C.PLAN_COUNTS)
        torch.manual_seed(1)
        seeds = ds.train_idx[:500]
        blocks = MultiLayerNeighborSampler([10, 10, 10]).sample_blocks(g, seeds, torch.Generator().manual_seed(8))
        labels = ds.labels[seeds, 0]
        out.append(_train_step(model, lambda: model(blocks), labels))
        assert (_C.PLAN_COUNTS["device_plan"] > c0["device_plan"]) == flag and (_C.PLAN_COUNTS["host_plan"] > c0["host_plan"]) == (not flag)
    _bit_identical(out[0], out[1], model)
