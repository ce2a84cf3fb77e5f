"""GraphSAINT node sets, loss weights and the weighted step without a GPU: the numpy restatement of the walk contract
(tests/saint_cases.py) is checked to be a walk with the stated distributions and to give the structure GraphSAINT batches are
chosen for; `saint_loss_weights`, the weighted tensor-op loss, `SAINTSampler` / `SAINTLoader` / `build_saint` on CPU graphs over
stand-ins for the new wrappers; the exported symbols and their argument checks.  tests/test_saint_gpu.py holds the kernels to the
restatement bit for bit."""
import ctypes
import math

import numpy as np
import pytest
import torch

import bot_amd
from bot_amd import synth
from bot_amd import train as T
from bot_amd.graph import reorder_graph
from tests import saint_cases as SN
from tests import subgraph_cases as SC


def _graph(n=300, e_raw=2500, seed=1, loops=True):
    rs, rd = synth.powerlaw_edges(n, e_raw, seed)
    g = bot_amd.to_bidirected(bot_amd.Graph(rs, rd, n)).remove_self_loop()      # no parallel edges
    return g.add_self_loop() if loops else g


def _csc(g):
    indptr, indices, _ = SC.csc_arrays(g)
    return indptr.astype(np.int64), indices.astype(np.int64)


@pytest.fixture
def standin(monkeypatch):
    from bot_amd import _C
    monkeypatch.setattr(_C, "node_subgraph", SC.node_subgraph_standin)
    monkeypatch.setattr(_C, "saint_walk", SN.saint_walk_standin)
    monkeypatch.setattr(_C, "saint_nodes", SN.saint_nodes_standin)


# ------------------------------------------------------------------------------------------------ 1. the restatement is a walk
@pytest.mark.parametrize("loops", [True, False])
def test_restatement_walks_along_edges(loops):
    rs, rd = synth.powerlaw_edges(400, 1500, 3)
    g = bot_amd.Graph(rs, rd, 400)                                              # raw directed edges: some nodes have no in-edge
    g = g.add_self_loop() if loops else g.remove_self_loop()
    indptr, indices = _csc(g)
    n = g.number_of_nodes()
    deg = np.diff(indptr)
    assert loops or (deg == 0).sum() > 0
    s, d = (t.numpy() for t in g.edges())
    edges = set(zip(s.tolist(), d.tolist()))
    nids = np.random.default_rng(0).permutation(n)[:37]
    stayed = 0
    for root_mode, ids in ((0, None), (0, nids), (1, None)):
        tr = SN.walk_reference(indptr, indices, ids, 500, 4, root_mode, 11)
        assert tr.shape == (500, 5) and tr.dtype == np.int32 and tr.min() >= 0 and tr.max() < n
        if ids is not None:
            assert set(tr[:, 0].tolist()) <= set(ids.tolist())                  # roots lie in nids
        for t in range(1, 5):
            for u, v in zip(tr[:, t].tolist(), tr[:, t - 1].tolist()):          # (source, destination): the edge the message takes
                if deg[v] == 0:
                    assert u == v
                    stayed += 1
                else:
                    assert (u, v) in edges
        assert np.array_equal(tr, SN.walk_reference(indptr, indices, ids, 500, 4, root_mode, 11))
        assert not np.array_equal(tr, SN.walk_reference(indptr, indices, ids, 500, 4, root_mode, 12))
        # a prefix of the walks and of the steps is a prefix of the trace: walk i at step t depends on (i, t, seed) alone
        assert np.array_equal(tr[:100, :3], SN.walk_reference(indptr, indices, ids, 100, 2, root_mode, 11))
    assert loops or stayed > 0
    tr0 = SN.walk_reference(indptr, indices, nids, 9, 0, 0, 5)
    assert tr0.shape == (9, 1)
    assert SN.walk_reference(indptr, indices, None, 0, 3, 0, 5).shape == (0, 4)
    assert np.array_equal(SN.node_set_reference(np.array([[5, 3, 5], [9, 3, 0]])), np.array([0, 3, 5, 9], dtype=np.int32))


# ------------------------------------------------------------------------------------------------ 2. distributions
def test_draws_have_the_stated_distributions():
    """Chi-square statistics under the 99.9th percentile of their degrees of freedom (21: 46.80, 39: 72.05, 49: 85.35), every cell
    expecting at least 50 hits.  Seeds 2024 / 2025 / 2026 were fixed before the first run and all three checks passed on them: no
    other seed was tried.  A failure here is first a finding about the draw (the counter packing i << 32 | t, the umulhi64
    range), and only after that the one case in a thousand."""
    g = _graph(n=50, e_raw=300, seed=5)
    indptr, indices = _csc(g)
    n, nnz = g.number_of_nodes(), len(indices)
    # (a) uniform roots over nids, with replacement
    nids = np.random.default_rng(1).permutation(n)[:40]
    R = 40 * 100
    roots = SN.walk_reference(indptr, indices, nids, R, 0, 0, 2024)[:, 0]
    obs = np.array([(roots == v).sum() for v in nids])
    assert obs.sum() == R
    chi2 = float(((obs - R / 40) ** 2 / (R / 40)).sum())
    print("roots", chi2)
    assert chi2 < 72.05, chi2
    # (b) root_mode 1: in proportion to the out-degree
    outdeg = np.bincount(indices, minlength=n)
    assert outdeg.min() >= 1
    R = int(math.ceil(50 * nnz / outdeg.min()))
    roots = SN.walk_reference(indptr, indices, None, R, 0, 1, 2025)[:, 0]
    obs = np.bincount(roots, minlength=n)
    exp = R * outdeg / nnz
    assert exp.min() >= 50
    chi2 = float(((obs - exp) ** 2 / exp).sum())
    print("degree-proportional", chi2, "R", R)
    assert chi2 < 85.35, chi2
    # (c) the first step from one fixed root (the node of this graph whose in-degree is nearest to 20 from above: 22): uniform over its
    # in-neighbours
    deg = np.diff(indptr)
    root = int(np.argmin(np.abs(deg - 20) + (deg < 20) * 1000))
    d = int(deg[root])
    assert d == 22, d
    R = 50 * d
    tr = SN.walk_reference(indptr, indices, np.array([root]), R, 1, 0, 2026)
    assert np.all(tr[:, 0] == root)
    nbrs = indices[indptr[root]:indptr[root + 1]]
    assert len(set(nbrs.tolist())) == d
    obs = np.array([(tr[:, 1] == u).sum() for u in nbrs])
    assert obs.sum() == R
    chi2 = float(((obs - R / d) ** 2 / (R / d)).sum())
    print("first step", chi2)
    assert chi2 < 46.80, chi2


# ------------------------------------------------------------------------------------------------ 3. structure
def test_walk_batches_keep_the_edges_they_were_reached_by():
    """Preprocessed (bidirected, self-looped) power-law graph, walk mode with R = N / 80, L = 2: the induced subgraph holds at least
    2 (n - r) edges that are not self-loops, n its nodes and r its distinct roots - every node a walk reaches beyond the roots keeps
    the edge pair to the node it was first reached from, and those pairs are distinct.  Exact, not a tolerance."""
    n_nodes = 20000
    ratios = []
    for s in range(8):
        rs, rd = synth.powerlaw_edges(n_nodes, 137000, s)
        g = bot_amd.preprocess(bot_amd.Graph(rs, rd, n_nodes))
        indptr, indices, eid = SC.csc_arrays(g)
        tr = SN.walk_reference(indptr, indices, None, n_nodes // 80, 2, 0, 100 + s)
        nodes = SN.node_set_reference(tr)
        n, r = len(nodes), len(np.unique(tr[:, 0]))
        off, src, _ = SC.induced_reference(indptr, indices, eid, nodes)
        dst = np.repeat(np.arange(n), np.diff(off))
        non_loop = int((src != dst).sum())
        assert non_loop >= 2 * (n - r), (s, non_loop, n, r)
        rnd = np.random.default_rng(s).permutation(n_nodes)[:n]
        off2, src2, _ = SC.induced_reference(indptr, indices, eid, rnd)
        ratios.append(non_loop / max(1, int((src2 != np.repeat(np.arange(n), np.diff(off2))).sum())))
    print("non-loop edges against a random set of equal size:", [round(x, 1) for x in ratios])        # reported, not asserted


# ------------------------------------------------------------------------------------------------ 4. loss weights
@pytest.mark.parametrize("reordered", [False, True])
def test_loss_weights_equal_the_restatement_and_unbias_the_presample(standin, reordered):
    from bot_amd.sampling import SAINTSampler, saint_loss_weights
    g = _graph(n=900, e_raw=7000, seed=2)
    if reordered:
        g = reorder_graph(g, "degree")
    n = g.number_of_nodes()
    for sampler in (SAINTSampler("walk", (12, 2)), SAINTSampler("node", 40), SAINTSampler("walk", (10, 3), nids=torch.arange(0, n, 7))):
        K = 25
        lw = saint_loss_weights(g, sampler, K, seed=3)
        want, sets, count = SN.loss_weights_reference(g, sampler, K, seed=3)
        assert lw.dtype == torch.float32 and lw.shape == (n,)
        assert np.array_equal(lw.numpy(), want)
        assert torch.equal(lw, saint_loss_weights(g, sampler, K, seed=3))                       # a pure function of its arguments
        assert not torch.equal(lw, saint_loss_weights(g, sampler, K, seed=4))
        assert (count == 0).sum() > 0 and np.all(want[count == 0] == K)                          # never visited: n_presample
        assert np.array_equal(want[count > 0], (np.float32(K) / count[count > 0].astype(np.float32)))
        # the identity the normalisation exists for: the pre-sample mean of the weighted batch sums is the sum over the visited nodes
        x = np.random.default_rng(0).standard_normal(n)
        lw64 = K / np.maximum(count, 1).astype(np.float64)
        mean = sum(float((lw64[s] * x[s]).sum()) for s in sets) / K
        assert abs(mean - float(x[count > 0].sum())) <= 1e-9 * float(np.abs(x).sum())
        np.testing.assert_allclose(lw.numpy().astype(np.float64), lw64, rtol=1e-6)
    with pytest.raises(ValueError):
        saint_loss_weights(g, SAINTSampler("node", 40), 0)


# ------------------------------------------------------------------------------------------------ 5. the weighted loss
def _loss_problem(n=203, C=7, seed=0):
    gen = torch.Generator().manual_seed(seed)
    pred = (2 * torch.randn(n, C, generator=gen, dtype=torch.float64)).requires_grad_()
    labels = torch.randint(0, C, (n, 1), generator=gen)
    wn = (torch.rand(n, generator=gen) < 0.4).float()
    labels[wn == 0] = -1                                                                         # placeholders outside the prediction set
    lw = 0.5 + 3.5 * torch.rand(n, generator=gen, dtype=torch.float64)
    return pred, labels, wn, lw


@pytest.mark.parametrize("kind", ["logit", "loge", "savage"])
def test_weighted_tensor_op_loss_against_the_formula(kind):
    pred, labels, wn, lw = _loss_problem()
    assert int((wn == 0).sum()) > 0 and int(labels[wn == 0].max()) == -1
    got = T.weighted_node_loss(pred, labels, wn, lw, kind)
    (g_got,) = torch.autograd.grad(got, pred)
    got = got.detach()
    want = SN.weighted_loss_formula(pred, labels, wn, lw, kind, T.EPSILON)
    (g_want,) = torch.autograd.grad(want, pred)
    want = want.detach()
    assert got.dtype == torch.float64
    assert abs(float(got) - float(want)) <= 1e-12 * abs(float(want))
    assert float((g_got - g_want).abs().max()) <= 1e-12 * float(g_want.abs().max())
    assert not g_got[wn == 0].any() and bool(torch.isfinite(g_got).all())
    # lw = 1: today's expression
    ones = torch.ones_like(lw)
    y = T.per_node_loss(pred, labels.clamp(0, pred.shape[1] - 1), kind)
    today = torch.where(wn > 0, y, torch.zeros_like(y)).sum() / wn.sum()
    unit = T.weighted_node_loss(pred, labels, wn, ones, kind)
    (g_unit,), (g_today,) = torch.autograd.grad(unit, pred), torch.autograd.grad(today, pred)
    unit, today = unit.detach(), today.detach()
    assert abs(float(unit) - float(today)) <= 1e-12 * abs(float(today))
    assert float((g_unit - g_today).abs().max()) <= 1e-12 * float(g_today.abs().max())
    # a constant weight changes nothing (self-normalised), a varying one does
    assert abs(float(T.weighted_node_loss(pred, labels, wn, 3 * ones, kind).detach()) - float(today)) <= 1e-12 * abs(float(today))
    assert abs(float(got) - float(today)) > 1e-6


def node_loss_weighted_standin(x, labels, wn, lw, wsum, kind, eps, want_grad=True):
    """_C.node_loss_weighted on CPU tensors: the contract of bot_node_loss_weighted_f32 over the emulated node_loss."""
    from tests import _oracle_backend as OB
    y, dx = OB.node_loss(x, labels, wn, wsum, kind, eps, want_grad)
    y[:x.shape[0]] *= lw
    return y, None if dx is None else dx * lw[:, None]


@pytest.mark.parametrize("stack", ["gat", "gcn"])
def test_weighted_train_step_on_the_emulated_backend(golden, monkeypatch, stack):
    import torch.nn.functional as F
    from bot_amd import _C, nn as bnn
    from tests import _oracle_backend
    _oracle_backend.install(monkeypatch)
    monkeypatch.setattr(_C, "node_loss_weighted", node_loss_weighted_standin)
    s, d, n = golden.graph("g300")
    g = bot_amd.Graph(s, d, n)
    C, fin = 5, 9
    gen = torch.Generator().manual_seed(7)
    feat = torch.randn(n, fin, generator=gen)
    labels = torch.randint(0, C, (n, 1), generator=gen)
    perm = torch.randperm(n, generator=gen)
    tr, va, te = perm[: n // 2], perm[n // 2: 3 * n // 4], perm[3 * n // 4:]
    mask = torch.rand(tr.shape, generator=gen) < 0.5
    lw = 0.5 + 3.5 * torch.rand(n, generator=gen)

    def run(fused_step, loss_weight):
        torch.manual_seed(3)
        if stack == "gat":
            model = bnn.GAT(dim_node=fin + C, dim_edge=0, dim_output=C, n_hidden=16, n_layers=3, n_heads=3, activation=F.relu, norm="batch",
                            linear=True)
        else:
            model = bnn.GCN(in_feats=fin + C, n_classes=C, n_hidden=16, n_layers=3, activation=F.relu, norm="batch", norm_adj="symm",
                            use_linear=True)
        opt = torch.optim.SGD(model.parameters(), lr=0.0)
        monkeypatch.setattr(T, "FUSED_STEP", fused_step)
        loss, pred = T.train_step(model, g, feat, labels, tr, va, te, opt, use_labels=True, loss="loge", n_classes=C, mask=mask,
                                  loss_weight=loss_weight)
        return float(loss), pred.detach(), {k: p.grad.clone() for k, p in model.named_parameters()}
    from tests.parity_cases import grad_close
    plain, _, _ = run(True, None)
    fused_loss, pred, grads = run(True, lw)
    tensor_loss, pred_t, grads_t = run(False, lw)
    assert math.isfinite(fused_loss) and abs(fused_loss - plain) > 1e-6                          # the weights reach the loss
    assert abs(fused_loss - tensor_loss) <= 2e-6 * max(1.0, abs(tensor_loss))                    # the two forms of the weighted step agree
    for k in grads:
        grad_close(grads[k], grads_t[k].numpy())
    # the loss is the formula on the step's own logits and prediction nodes
    wn = torch.zeros(n)
    wn[tr] = (~mask).float()
    want = SN.weighted_loss_formula(pred.double(), labels, wn, lw.double(), "loge", T.EPSILON)
    assert abs(fused_loss - float(want)) <= 2e-6 * max(1.0, abs(float(want)))
    ones_loss, _, _ = run(True, torch.ones(n))
    assert abs(ones_loss - plain) <= 2e-6 * max(1.0, abs(plain))
    with pytest.raises(ValueError):
        run(True, lw[:-1])


def test_subgraph_step_slices_the_weights_for_both_kinds_of_stack(standin, monkeypatch):
    """`minibatch.subgraph_step(loss_weight=...)`: the GCN / GAT stacks get the batch's slice as `loss_weight`; the edge-feature
    stacks weight their per-node loss under the same self-normalised mean (lw = 1: today's .mean())."""
    from bot_amd import minibatch
    from bot_amd.sampling import SAINTSampler
    g = _graph(n=400, e_raw=3000, seed=6)
    n = g.number_of_nodes()
    gen = torch.Generator().manual_seed(1)
    g.ndata["feat"] = torch.randn(n, 5, generator=gen)
    labels = torch.randint(0, 3, (n, 1), generator=gen)
    roles = minibatch.node_roles(n, torch.arange(0, n, 2))
    lw = 0.5 + torch.rand(n, generator=gen)
    sub = SAINTSampler("walk", (20, 2)).sample(g, 5)
    seen = {}

    def fake_train_step(model, graph, feat, y, tr, va, te, opt, **kw):
        seen.update(kw)
        return torch.zeros(()), None
    monkeypatch.setattr(T, "train_step", fake_train_step)
    minibatch.subgraph_step(None, sub, None, labels, roles, step_kw={"use_labels": False}, loss_weight=lw)
    assert torch.equal(seen["loss_weight"], lw[sub.parent_rows])
    seen.clear()
    minibatch.subgraph_step(None, sub, None, labels, roles, step_kw={"use_labels": False})
    assert "loss_weight" not in seen
    lin = torch.nn.Linear(5, 3)
    model = lambda s: lin(s.ndata["feat"])                                                     # noqa: E731
    model.train = lambda: None
    opt = torch.optim.SGD(lin.parameters(), lr=0.0)
    node_loss = lambda x, y: torch.nn.functional.cross_entropy(x, y[:, 0], reduction="none")   # noqa: E731
    plain = minibatch.subgraph_step(model, sub, opt, labels, roles, node_loss=node_loss)
    unit = minibatch.subgraph_step(model, sub, opt, labels, roles, node_loss=node_loss, loss_weight=torch.ones(n))
    weighted = minibatch.subgraph_step(model, sub, opt, labels, roles, node_loss=node_loss, loss_weight=lw)
    assert abs(float(plain[0]) - float(unit[0])) <= 1e-6 and plain[2] == unit[2] == weighted[2]
    rows = sub.parent_rows
    tr = torch.nonzero(roles[rows] == 1).squeeze(1)
    per = node_loss(lin(sub.ndata["feat"])[tr], labels[rows][tr])
    w = lw[rows][tr]
    assert abs(float(weighted[0]) - float((w * per).sum() / w.sum())) <= 1e-6
    assert abs(float(weighted[0]) - float(plain[0])) > 1e-6


# ------------------------------------------------------------------------------------------------ 6. surface
def test_sampler_and_loader_surface(standin):
    from bot_amd.sampling import SAINTLoader, SAINTSampler, Subgraph
    with pytest.raises(NotImplementedError, match="out of scope"):
        SAINTSampler("edge", 100)
    with pytest.raises(ValueError):
        SAINTSampler("metis", 100)
    with pytest.raises(ValueError):
        SAINTSampler("node", 100, nids=torch.arange(5))
    with pytest.raises(ValueError):
        SAINTSampler("walk", (-1, 2))
    g = _graph(n=700, e_raw=5000, seed=3)
    n = g.number_of_nodes()
    for sampler in (SAINTSampler("walk", (15, 2)), SAINTSampler("node", 50), SAINTSampler("walk", (15, 1), nids=torch.arange(100, 200))):
        nodes = sampler.sample_nodes(g, 9)
        assert nodes.dtype == torch.int32 and nodes.device == g.device
        assert np.array_equal(nodes.numpy(), SN.sampler_nodes_reference(g, sampler, 9))
        assert torch.all(nodes[1:] > nodes[:-1])                                                 # ascending, duplicate-free
        assert 0 < nodes.numel() <= sampler.n_roots * (sampler.length + 1)
        sub = sampler.sample(g, 9)
        assert isinstance(sub, Subgraph) and torch.equal(sub.parent_nid, nodes)
        off, src, pe = SC.induced_reference(*SC.csc_arrays(g), nodes.numpy())
        assert torch.equal(sub.csc.indptr.long(), torch.from_numpy(off)) and torch.equal(sub.csc.indices, torch.from_numpy(src))
        assert torch.equal(sub.parent_eid, torch.from_numpy(pe))
    assert SAINTSampler("walk", (0, 2)).sample_nodes(g, 1).numel() == 0
    with pytest.raises(ValueError, match="out of range"):
        SAINTSampler("walk", (3, 1), nids=torch.tensor([0, n])).sample_nodes(g, 1)
    # blocks and partitions
    s, d = g.edges()
    keep = d < 100
    block = bot_amd.Graph(s[keep], d[keep], n, num_dst_nodes=100)
    part = _graph(n=200, e_raw=1500, seed=7)
    part.halo = object()
    for bad in (block, part):
        with pytest.raises(ValueError, match="whole graph"):
            SAINTSampler("node", 10).sample_nodes(bad, 0)
        with pytest.raises(ValueError, match="whole graph"):
            SAINTLoader(bad, SAINTSampler("node", 10), 3)
    # the loader: same seed, same batches
    sampler = SAINTSampler("walk", (15, 2))
    loader = SAINTLoader(g, sampler, 6, seed=3)
    assert len(loader) == 6 and loader.g is g
    a = [b.clone() for b in SAINTLoader(g, sampler, 6, seed=3).node_batches()]
    b = [b.clone() for b in SAINTLoader(g, sampler, 6, seed=3).node_batches()]
    c = [b.clone() for b in SAINTLoader(g, sampler, 6, seed=4).node_batches()]
    assert len(a) == 6 and all(torch.equal(x, y) for x, y in zip(a, b))
    assert not any(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a, c))
    assert not any(x.shape == y.shape and torch.equal(x, y) for x, y in zip(a[:-1], a[1:]))   # every batch its own seed
    first = list(loader)
    second = list(loader)                                                                        # the next epoch draws on
    assert len(first) == 6 and all(isinstance(s_, Subgraph) for s_ in first)
    assert all(torch.equal(s_.parent_nid, x) for s_, x in zip(first, a))
    assert not all(x.parent_nid.shape == y.parent_nid.shape and torch.equal(x.parent_nid, y.parent_nid) for x, y in zip(first, second))
    # the per-batch seeds are drawn as MultiLayerNeighborSampler.sample_blocks draws a layer's
    seeds = SN.presample_seeds(6, 3)
    assert all(np.array_equal(x.numpy(), SN.sampler_nodes_reference(g, sampler, s_)) for x, s_ in zip(a, seeds))
    with pytest.raises(ValueError):
        SAINTLoader(g, sampler, 0)


def test_build_saint_names_and_defaults():
    from bot_amd import workloads
    with pytest.raises(ValueError):
        workloads.build_saint("citeseer", "cpu")
    with pytest.raises(ValueError):
        workloads.saint_defaults("arxiv", 1000, mode="edge")
    assert workloads.SAINT_COVERAGE == 50
    for name, n_batches in workloads.CLUSTERED.items():
        N = synth.SHAPES[name][0]
        for length in (2, 3):
            budget, nb, npre = workloads.saint_defaults(name, N, mode="walk", length=length)
            assert nb == n_batches and npre == 50 * n_batches
            assert budget == (math.ceil(N / (n_batches * (length + 1))), length)
            assert budget[0] * (length + 1) >= math.ceil(N / n_batches) > (budget[0] - 1) * (length + 1)
        budget, nb, npre = workloads.saint_defaults(name, N, mode="node")
        assert budget == math.ceil(N / n_batches) and nb == n_batches and npre == 50 * n_batches
        assert workloads.saint_defaults(name, N, n_batches=7, n_presample=11)[1:] == (7, 11)


# ------------------------------------------------------------------------------------------------ 7. symbols
def test_saint_symbols_are_exported_and_validate_arguments():
    from bot_amd import _C
    lib = _C._lib
    for name in ("bot_saint_walk_i32", "bot_saint_nodes_mark_i32", "bot_saint_nodes_list_i32", "bot_node_loss_weighted_f32"):
        assert name in _C.EXPORTED and hasattr(lib, name)
    assert lib.bot_abi_version() == 19
    buf = (ctypes.c_int32 * 16)()
    off = (ctypes.c_int64 * 16)()
    p, o = ctypes.addressof(buf), ctypes.addressof(off)
    walk = lib.bot_saint_walk_i32
    # NULL pointers -> BOT_E_NULL
    assert walk(None, p, 4, 8, None, 0, 3, 2, 0, 7, p, None) == -1
    assert walk(p, None, 4, 8, None, 0, 3, 2, 0, 7, p, None) == -1
    assert walk(p, p, 4, 8, None, 0, 3, 2, 0, 7, None, None) == -1 and b"saint_walk" in lib.bot_last_error()
    # sizes -> BOT_E_RANGE
    assert walk(p, p, -4, 8, None, 0, 3, 2, 0, 7, p, None) == -2
    assert walk(p, p, 4, -8, None, 0, 3, 2, 0, 7, p, None) == -2
    assert walk(p, p, 4, 8, None, 0, -3, 2, 0, 7, p, None) == -2
    assert walk(p, p, 4, 8, None, 0, 3, -1, 0, 7, p, None) == -2
    assert walk(p, p, 4, 8, p, -1, 3, 2, 0, 7, p, None) == -2
    assert walk(p, p, 4, 8, None, 0, 2 ** 29, 3, 0, 7, p, None) == -2                 # R (L + 1) = 2^31
    assert walk(p, p, 4, 8, None, 0, 2 ** 62, 3, 0, 7, p, None) == -2                 # ... also where the product wraps
    assert walk(p, p, 4, 8, None, 0, 3, 2, 2, 7, p, None) == -2                       # no such root mode
    assert walk(p, p, 4, 8, p, 2, 3, 2, 1, 7, p, None) == -2                          # degree-proportional roots take no nids
    assert walk(p, p, 4, 0, None, 0, 3, 2, 1, 7, p, None) == -2                       # ... and at least one edge
    assert walk(p, p, 4, 8, p, 0, 3, 2, 0, 7, p, None) == -2                          # roots asked of an empty node set
    assert walk(p, p, 0, 0, None, 0, 3, 2, 0, 7, p, None) == -2
    # no roots: a no-op, nothing launched, so no GPU is needed
    assert walk(p, None, 4, 8, None, 0, 0, 2, 0, 7, None, None) == 0
    mark, lst = lib.bot_saint_nodes_mark_i32, lib.bot_saint_nodes_list_i32
    assert mark(None, 6, p, 4, o, o, None) == -1
    assert mark(p, 6, None, 4, o, o, None) == -1
    assert mark(p, 6, p, 4, None, o, None) == -1
    assert mark(p, 6, p, 4, o, None, None) == -1
    assert mark(p, -6, p, 4, o, o, None) == -2 and mark(p, 6, p, -4, o, o, None) == -2
    assert mark(None, 0, p, 4, None, o, None) == 0
    assert lst(None, 4, o, 2, p, None) == -1
    assert lst(p, 4, None, 2, p, None) == -1
    assert lst(p, 4, o, 2, None, None) == -1
    assert lst(p, 4, o, 5, p, None) == -2 and lst(p, 4, o, -1, p, None) == -2 and b"saint_nodes_list" in lib.bot_last_error()
    assert lst(p, 4, None, 0, None, None) == 0
    f = lib.bot_node_loss_weighted_f32
    P = 4096        # any non-NULL value: every refusal happens before a launch

    def loss(x=P, ldx=7, n=10, C=7, labels=P, ldl=1, wn=P, lw=P, wsum=P, kind=0, eps=0.3, y=P, n_pad=64, dx=P, lddx=7):
        return f(x, ldx, n, C, labels, ldl, wn, lw, wsum, kind, eps, y, n_pad, dx, lddx, None)
    assert loss(C=129) == -2 and b"node_loss_weighted" in lib.bot_last_error()
    assert loss(C=0) == -2 and loss(kind=3) == -2 and loss(n=-1) == -2 and loss(n_pad=9) == -2 and loss(lddx=6) == -2 and loss(ldx=6) == -2
    for name in ("x", "labels", "wn", "lw", "wsum", "y"):
        assert loss(**{name: None}) == -1, name
    assert loss(n=0, n_pad=0) == 0
    # the wrappers refuse CPU tensors: there is no fallback
    with pytest.raises(_C.BotKernelError):
        _C.node_loss_weighted(torch.zeros(4, 3), torch.zeros(4, 1, dtype=torch.int64), torch.ones(4), torch.ones(4), torch.ones(1), "logit", 0.3)
    g = _graph(n=50, e_raw=300, seed=5)
    with pytest.raises(_C.BotKernelError):
        _C.saint_walk(g.csc, None, 4, 2, 0, 1)
    with pytest.raises(_C.BotKernelError):
        _C.saint_nodes(torch.zeros(4, dtype=torch.int32), torch.full((50,), -1, dtype=torch.int32))


def test_nids_are_checked_against_every_graph_the_sampler_meets(standin):
    from bot_amd.sampling import SAINTSampler
    big, small = _graph(n=700, e_raw=5000, seed=3), _graph(n=200, e_raw=1500, seed=7)
    sampler = SAINTSampler("walk", (5, 1), nids=torch.tensor([3, 650]))
    assert sampler.sample_nodes(big, 1).numel() > 0
    with pytest.raises(ValueError, match="out of range"):
        sampler.sample_nodes(small, 1)                                                          # the copy made for `big` is not reused
    assert sampler.sample_nodes(big, 1).numel() > 0


def test_bench_saint_child_runs_on_the_emulated_backend(standin, monkeypatch):
    """tools/bench_saint.py's child: a SAINT and a clustered workload of S-cora (scale 0.3) in one process, alternating, on CPU
    tensors over the emulated kernels - the five-way split adds up, the counts are those of the batches, the line is JSON."""
    import importlib.util
    import json
    import os
    import types
    from bot_amd import _C, workloads
    from tests import _oracle_backend
    _oracle_backend.install(monkeypatch)
    monkeypatch.setattr(_C, "node_loss_weighted", node_loss_weighted_standin)
    for name, value in (("synchronize", None), ("reset_peak_memory_stats", None), ("max_memory_allocated", 0), ("get_device_name", "cpu")):
        monkeypatch.setattr(torch.cuda, name, lambda *a, _v=value, **k: _v)
    for name in ("build_saint", "build_clustered"):
        monkeypatch.setattr(workloads, name, lambda wl, dev, _f=getattr(workloads, name), **k: _f(wl, "cpu", **k))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("bench_saint", os.path.join(root, "tools", "bench_saint.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    out = tool.child("cora", types.SimpleNamespace(scale=0.3, seed=0, mode="walk", length=2, rounds=2, max_batches=None))
    out = json.loads(json.dumps(out))
    n = out["n_nodes"]
    assert out["budget"] == [math.ceil(n / 15), 2] and out["n_batches"] == 5 and out["presample_sets"] == 250
    for side in ("saint", "clustered"):
        s = out[side]
        assert len(s["rounds"]) == 2 and set(s["split_ms_per_batch_median"]) == set(tool.KEYS)
        for r in s["rounds"]:
            assert r["batches"] == 5 and r["skipped"] == 0
            assert abs(sum(r["split_ms_per_batch"].values()) - r["ms_per_batch"]) < 0.01
            assert 0 < r["non_loop_edges_per_batch"] <= r["edges_per_batch"] - 1 and r["nodes_per_batch"] <= math.ceil(n / 5)
    # the claim the tool exists to measure, at this small scale: a SAINT batch keeps more non-loop edges than a cluster part
    assert out["saint"]["non_loop_edges_per_batch_median"] > out["clustered"]["non_loop_edges_per_batch_median"]
