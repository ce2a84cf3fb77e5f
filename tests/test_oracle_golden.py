"""Pin the oracle (oracle/ref_models.py, oracle/ref_ops.py) against the golden vectors that were
produced by executing the reference's own modules (oracle/gen_golden.py) and against the
known-answer material the reference itself holds (GraphConv docstring rows, parameter counts)."""
import ast

import numpy as np
import pytest
import torch

from oracle import ref_models as RM
from oracle import ref_ops as R
from oracle.ref_models import CooGraph

TOL = {"float32": dict(rtol=2e-5, atol=2e-6), "float64": dict(rtol=1e-11, atol=1e-12)}


def close(a, b, dt="float32", scale=1.0):
    a = a.detach().numpy() if torch.is_tensor(a) else np.asarray(a)
    tol = TOL[dt]
    np.testing.assert_allclose(a, b, rtol=tol["rtol"] * scale, atol=tol["atol"] * scale * max(1.0, float(np.abs(b).max())))


def coo(golden, name):
    s, d, n = golden.graph(name)
    return CooGraph(s, d, n)


# ------------------------------------------------------------------ integer work: bit-exact
def test_preprocess_bit_exact(golden):
    for name in ("g64", "g300"):
        rs, rd, n = golden.graph(name + "_raw")
        s, d = R.preprocess_edges(rs, rd, n)
        es, ed, _ = golden.graph(name)
        assert torch.equal(s, es) and torch.equal(d, ed)
        # self-loop edge ids are the last N (run.py:143)
        assert torch.equal(s[-n:], torch.arange(n)) and torch.equal(d[-n:], torch.arange(n))
        f = golden.file("graphs")
        assert np.array_equal(R.in_degrees(d, n).numpy(), f[f"{name}.in_deg"])
        assert np.array_equal(R.out_degrees(s, n).numpy(), f[f"{name}.out_deg"])
        # symmetric after to_bidirected: in == out degrees
        assert np.array_equal(f[f"{name}.in_deg"], f[f"{name}.out_deg"])


def test_csc_csr_consistent(golden):
    s, d, n = golden.graph("g300")
    indptr, indices, eid = R.build_csc(s, d, n)
    assert indptr[-1] == s.numel()
    assert torch.equal(indices, s[eid])
    assert torch.equal(torch.repeat_interleave(torch.arange(n), indptr[1:] - indptr[:-1]), d[eid])
    for v in range(n):  # stable in edge id
        seg = eid[indptr[v]:indptr[v + 1]]
        assert torch.all(seg[1:] > seg[:-1])


# ------------------------------------------------------------------ the reference's own known answers
def test_graphconv_docstring_known_answer(golden):
    """models.py:186-209: feat = ones, random W — every row is s_i * (1^T W), so rows are pinned up to
    the common vector.  Pins degrees, clamp(min=1), both ^-0.5 scalings and the sum aggregation."""
    f = golden.file("graphconv")
    for gname, key in (("doc_loop", "doc.case1"), ("doc_noloop", "doc.case2")):
        g = coo(golden, gname)
        w = torch.randn(10, 2, dtype=torch.float64)
        rst = RM.graphconv_forward(g, torch.ones(6, 10, dtype=torch.float64), w, None, "both",
                                   allow_zero_in_degree=True).numpy()
        col = w.sum(0).numpy()
        scale = rst / col  # per-row scalar s_i, same in both columns
        assert np.allclose(scale[:, 0], scale[:, 1])
        printed = f[key]
        ref_scale = printed[:, 0] / printed[1, 0]  # row 1 has s = 1 in both examples
        np.testing.assert_allclose(scale[:, 0] / scale[1, 0], ref_scale, atol=2e-4)


def test_zero_in_degree_guard(golden):
    g = coo(golden, "doc_noloop")  # node 5 has no in-edge
    with pytest.raises(RM.ZeroInDegreeError):
        RM.graphconv_forward(g, torch.ones(6, 3), torch.ones(3, 2), None)


def test_param_counts_recorded_by_reference(golden):
    f = golden.file("stacks")
    assert int(f["count.arxiv_gat_cfg2"]) == 1441580  # run.py:1009
    assert int(f["count.arxiv_gcn_h256"]) == 109608  # run.py:828
    assert int(golden.file("proteins")["count.proteins_gat"]) == 2475232  # ogbn-proteins/gat.py:377


# ------------------------------------------------------------------ layers vs fixtures
def _backward(out, gout, inputs):
    return torch.autograd.grad((out * gout).sum(), inputs, allow_unused=True)


def test_graphconv_matches_reference(golden):
    for c in golden.cases("graphconv"):
        gname, norm, fin, fout, dt = c["meta"]
        g = coo(golden, str(gname))
        p = c.params()
        feat = c.t("feat").requires_grad_()
        rst = RM.graphconv_forward(g, feat, p["weight"], p["bias"], str(norm))
        close(rst, c["rst"], dt)
        dfeat, dw, db = _backward(rst, c.t("gout"), [feat, p["weight"], p["bias"]])
        close(dfeat, c["dfeat"], dt, 4)
        close(dw, c["g.weight"], dt, 4)
        close(db, c["g.bias"], dt, 4)


def test_gatconv_matches_reference(golden):
    n_drop = 0
    for c in golden.cases("gatconv"):
        gname, symm, attn_r, linear, H, D, fin, edge_drop, dt = c["meta"]
        g = coo(golden, str(gname))
        p = c.params()
        feat = c.t("feat").requires_grad_()
        keep = c.t("keep_eids") if "keep_eids" in c else None
        n_drop += keep is not None
        rst = RM.gatconv_forward(g, feat, p["fc.weight"], p["attn_l"], p.get("attn_r"), p.get("res_fc.weight"),
                                 num_heads=int(H), out_feats=int(D), use_symmetric_norm=bool(int(symm)),
                                 keep_eids=keep)
        close(rst, c["rst"], dt, 2)
        names = [k for k in p if f"g.{k}" in c]
        grads = _backward(rst, c.t("gout"), [feat] + [p[k] for k in names])
        close(grads[0], c["dfeat"], dt, 8)
        for k, gr in zip(names, grads[1:]):
            close(gr, c[f"g.{k}"], dt, 8)
    assert n_drop >= 4  # the edge-drop branch (models.py:528-539) is covered


def _stack_forward(g, c):
    gname, kind, training, cfg = c["meta"]
    cfg = ast.literal_eval(str(cfg))
    p = c.params()
    feat = c.t("feat").requires_grad_()
    training = bool(int(training))
    if kind == "gcn":
        logits = RM.gcn_forward(g, feat, p, n_layers=cfg["n_layers"], norm=cfg["norm"], norm_adj=cfg["norm_adj"],
                                use_linear=cfg["use_linear"], residual=cfg["residual"], training=training)
    else:
        logits = RM.gat_forward(g, feat, p, n_layers=cfg["n_layers"], n_heads=cfg["n_heads"],
                                n_hidden=cfg["n_hidden"], n_classes=5, norm=cfg["norm"],
                                non_interactive_attn=cfg["non_interactive_attn"],
                                use_symmetric_norm=cfg["use_symmetric_norm"], linear=cfg["linear"],
                                residual=cfg["residual"], training=training)
    return logits, feat, p


def test_stacks_match_reference(golden):
    for c in golden.cases("stacks"):
        g = coo(golden, str(c["meta"][0]))
        logits, feat, p = _stack_forward(g, c)
        close(logits, c["logits"], "float32", 8)
        names = [k for k in p if f"g.{k}" in c]
        grads = _backward(logits, c.t("gout"), [feat] + [p[k] for k in names])
        close(grads[0], c["dfeat"], "float32", 50)
        for k, gr in zip(names, grads[1:]):
            close(gr, c[f"g.{k}"], "float32", 50)
        assert sum(v.numel() for k, v in p.items() if "running_" not in k and "num_batches" not in k) == int(c["n_params"])


def test_proteins_layer_and_stack_match_reference(golden):
    for c in golden.cases("proteins", count_key="n_conv_cases"):
        gname, edge_feats, use_attn_dst, edge_drop, H, D = c["meta"]
        g = coo(golden, str(gname))
        p = c.params()
        feat = c.t("feat").requires_grad_()
        ef = c.t("efeat").requires_grad_() if "efeat" in c else None
        keep = c.t("keep_eids") if "keep_eids" in c else None
        rst = RM.proteins_gatconv_forward(g, feat, p, "", n_heads=int(H), out_feats=int(D), feat_edge=ef, keep_eids=keep)
        close(rst, c["rst"], "float32", 4)
        names = [k for k in p if f"g.{k}" in c]
        ins = [feat] + ([ef] if ef is not None else []) + [p[k] for k in names]
        grads = list(_backward(rst, c.t("gout"), ins))
        close(grads.pop(0), c["dfeat"], "float32", 8)
        if ef is not None:
            close(grads.pop(0), c["defeat"], "float32", 8)
        for k, gr in zip(names, grads):
            close(gr, c[f"g.{k}"], "float32", 8)
    f = golden.file("proteins")
    g = coo(golden, "g64")
    for training in (0, 1):
        pre = f"s{training}."
        from tests._golden import Case
        c = Case({k[len(pre):]: v for k, v in f.items() if k.startswith(pre)})
        p = c.params()
        logits = RM.proteins_gat_forward(g, c.t("nfeat"), c.t("efeat"), p, n_layers=2, n_heads=2, n_hidden=5,
                                         training=bool(training))
        close(logits, c["logits"], "float32", 8)
        names = [k for k in p if f"g.{k}" in c]
        grads = _backward(logits, c.t("gout"), [p[k] for k in names])
        for k, gr in zip(names, grads):
            if gr is not None:
                close(gr, c[f"g.{k}"], "float32", 50)


def test_products_stack_matches_reference(golden):
    """`GAT` of src/ogbn-products/models.py:170-265 (no node encoder, residual flag, optional edge encoder), fixtures produced
    by executing that file."""
    f = golden.file("products")
    g = coo(golden, "g64")
    from tests._golden import Case
    for ci in range(int(f["n_cases"])):
        pre = f"s{ci}."
        c = Case({k[len(pre):]: v for k, v in f.items() if k.startswith(pre)})
        residual, edge_emb, training = (int(x) for x in c["meta"])
        p = c.params()
        logits = RM.proteins_gat_forward(g, c.t("nfeat"), c.t("efeat") if edge_emb else None, p, n_layers=3, n_heads=2,
                                         n_hidden=5, training=bool(training), use_node_encoder=False, residual=bool(residual))
        close(logits, c["logits"], "float32", 8)
        names = [k for k in p if f"g.{k}" in c]
        grads = _backward(logits, c.t("gout"), [p[k] for k in names])
        for k, gr in zip(names, grads):
            if gr is not None:
                close(gr, c[f"g.{k}"], "float32", 50)


# ------------------------------------------------------------------ callers (run.py)
def test_losses_and_add_labels_match_reference(golden):
    f = golden.file("train")
    x, y = torch.from_numpy(f["loss.x"]), torch.from_numpy(f["loss.y"])
    for ln in ("logit", "loge", "savage"):
        assert abs(RM.compute_loss(x, y, ln).item() - float(f[f"loss.{ln}"])) < 1e-6
    assert int(f["n_cases"]) == 5
    for ci in range(int(f["n_cases"])):
        k = f"t{ci}."
        feat, labels = torch.from_numpy(f[k + "feat"]), torch.from_numpy(f[k + "labels"])
        tr, mask = torch.from_numpy(f[k + "train_idx"]), torch.from_numpy(f[k + "mask"])
        aug = RM.add_labels(feat, labels, tr[mask], 4)
        assert np.array_equal(aug.numpy(), f[k + "aug"])  # exact 0/1 columns
    # adjust_learning_rate (run.py:246-249) as the reference's RMSprop saw it at epochs 25, 51, 50 and 1
    assert RM.warmup_lr(0.01, 25) == pytest.approx(float(f["t0.lr"]))
    assert RM.warmup_lr(0.01, 51) is None and float(f["t2.lr"]) == pytest.approx(0.01)
    assert RM.warmup_lr(0.01, 50) == pytest.approx(float(f["t3.lr"])) == pytest.approx(0.01)
    assert RM.warmup_lr(0.01, 1) == pytest.approx(float(f["t4.lr"])) == pytest.approx(0.0002)


def test_dgl_documented_known_answers():
    """THIRD-PARTY, RECALLED: the worked examples in DGL's own API documentation for the two operators whose arithmetic the
    reference fixtures cannot pin (dgl is absent; oracle/dgl_standin.py is the builder's).  They are written here from memory
    of the published docs of `dgl.nn.functional.edge_softmax` and `dgl.to_bidirected` (DGL 0.5-0.9 docstrings), not read from
    any file in this container — independent of the builder's reading of the semantics, but not machine-verified against dgl.

    edge_softmax: graph 0->0, 0->1, 0->2, 1->1, 1->2, 2->2 with unit logits; normalised by destination the documented result
    is [1, .5, .3333, .5, .3333, .3333].  to_bidirected: 0->1, 1->2, 2->0 becomes the six edges {(0,1),(1,2),(2,0),(1,0),(2,1),(0,2)};
    the docs print them in concatenation order, the library's `to_simple` sorts by (src, dst) — only the SET is asserted, and
    edge ids are never compared against dgl's."""
    src, dst = torch.tensor([0, 0, 0, 1, 1, 2]), torch.tensor([0, 1, 2, 1, 2, 2])
    a = R.edge_softmax(dst, 3, torch.ones(6, 1))
    assert torch.allclose(a.squeeze(1), torch.tensor([1.0, 0.5, 1 / 3, 0.5, 1 / 3, 1 / 3]), atol=1e-4)
    from oracle import c_ops
    g = c_ops.CGraph(src, dst, 3)
    assert torch.allclose(c_ops.edge_softmax(g, torch.ones(6, 1, 1), None).reshape(-1), a.squeeze(1), atol=1e-6)
    # and the `eids` form (models.py:537): softmax over an edge-induced subgraph, here without edge 0->1 and 1->2
    eids = torch.tensor([0, 2, 3, 5])
    sub = R.edge_softmax(dst, 3, torch.ones(4, 1), eids)
    assert torch.allclose(sub.squeeze(1), torch.tensor([1.0, 0.5, 1.0, 0.5]), atol=1e-6)
    s2, d2 = R.to_bidirected(torch.tensor([0, 1, 2]), torch.tensor([1, 2, 0]), 3)
    assert set(zip(s2.tolist(), d2.tolist())) == {(0, 1), (1, 2), (2, 0), (1, 0), (2, 1), (0, 2)} and s2.numel() == 6
    # u_mul_e_sum / copy_u_sum on the same 6-edge graph, worked by hand: out[v] = sum_{u->v} w_uv x[u]
    x = torch.tensor([[1.0], [10.0], [100.0]])
    w = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0, 6.0]).view(6, 1)
    assert torch.equal(R.u_mul_e_sum(src, dst, 3, x, w), torch.tensor([[1.0], [42.0], [653.0]]))
    assert torch.equal(R.copy_u_sum(src, dst, 3, x), torch.tensor([[1.0], [11.0], [111.0]]))


def test_edge_softmax_properties():
    """No golden vector exists for edge_softmax (parity unpinned): check the defining properties."""
    torch.manual_seed(0)
    n, E = 50, 400
    dst = torch.randint(0, n, (E,))
    e = torch.randn(E, 3, 1, dtype=torch.float64) * 5
    a = R.edge_softmax(dst, n, e)
    s = torch.zeros(n, 3, 1, dtype=torch.float64).index_add(0, dst, a)
    has = torch.bincount(dst, minlength=n) > 0
    assert torch.allclose(s[has], torch.ones_like(s[has]))
    assert torch.allclose(R.edge_softmax(dst, n, e + 100.0), a)  # shift invariance per destination
    eids = torch.randperm(E)[100:]
    sub = R.edge_softmax(dst, n, e[eids], eids)
    s2 = torch.zeros(n, 3, 1, dtype=torch.float64).index_add(0, dst[eids], sub)
    has2 = torch.bincount(dst[eids], minlength=n) > 0
    assert torch.allclose(s2[has2], torch.ones_like(s2[has2]))


def test_oracle_against_scipy_sparse(golden):
    """A third, library-made restatement of the operators' arithmetic: SciPy's sparse matrices define SpMM unambiguously (parallel
    edges are summed when a COO matrix is converted, as DGL sums messages of a multigraph).  oracle/ref_ops.py and the C kernels
    (oracle/c_ops.py) must agree with `A^T x`, with the edge-weighted `A_w^T x`, and with a softmax taken over the stored entries of
    each column — on the golden graphs and on a random multigraph with duplicate edges.  (This pins the arithmetic, not DGL's
    conventions — edge-id order of `to_bidirected`, `eids` semantics — which stay anchored on the reference's call sites.)"""
    import scipy.sparse as sp
    from oracle import c_ops
    gen = torch.Generator().manual_seed(77)
    cases = [golden.graph("g64"), golden.graph("g300")]
    n = 50
    cases.append((torch.randint(0, n, (400,), generator=gen), torch.randint(0, n, (400,), generator=gen), n))   # duplicates, self-loops
    for s, d, n in cases:
        E = s.numel()
        H, D = 3, 5
        x = torch.randn(n, H, D, generator=gen, dtype=torch.float64)
        w = torch.rand(E, H, generator=gen, dtype=torch.float64)
        A = sp.coo_matrix((np.ones(E), (s.numpy(), d.numpy())), shape=(n, n)).tocsr()          # A[u, v] = multiplicity of u -> v
        ref = (A.T @ x.reshape(n, H * D).numpy()).reshape(n, H, D)
        np.testing.assert_allclose(R.copy_u_sum(s, d, n, x).numpy(), ref, rtol=1e-12, atol=1e-12)
        cg = c_ops.CGraph(s, d, n)
        np.testing.assert_allclose(c_ops.copy_u_sum(cg, x.float()).numpy(), ref, rtol=1e-5, atol=1e-5)
        for h in range(H):
            Aw = sp.coo_matrix((w[:, h].numpy(), (s.numpy(), d.numpy())), shape=(n, n)).tocsr()
            np.testing.assert_allclose(R.u_mul_e_sum(s, d, n, x, w.unsqueeze(-1))[:, h].numpy(), Aw.T @ x[:, h].numpy(), rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(R.copy_e_sum(d, n, w).numpy(),
                                   np.stack([np.bincount(d.numpy(), weights=w[:, h].numpy(), minlength=n) for h in range(H)], 1), rtol=1e-12)
        # edge_softmax: exp(e - max over the in-edges) / sum over the in-edges, per destination and head, with numpy's ufuncs
        e = torch.randn(E, H, 1, generator=gen, dtype=torch.float64) * 4
        a = R.edge_softmax(d, n, e).squeeze(-1).numpy()
        mx = np.full((n, H), -np.inf)
        np.maximum.at(mx, d.numpy(), e.squeeze(-1).numpy())
        ex = np.exp(e.squeeze(-1).numpy() - mx[d.numpy()])
        den = np.zeros((n, H))
        np.add.at(den, d.numpy(), ex)
        np.testing.assert_allclose(a, ex / den[d.numpy()], rtol=1e-12, atol=1e-15)
        np.testing.assert_allclose(c_ops.edge_softmax(cg, e.float()).squeeze(-1).numpy(), ex / den[d.numpy()], rtol=1e-5, atol=1e-6)
        assert np.array_equal(torch.bincount(d, minlength=n).numpy(), np.asarray(A.sum(0)).ravel().astype(np.int64))       # in-degrees
        assert np.array_equal(torch.bincount(s, minlength=n).numpy(), np.asarray(A.sum(1)).ravel().astype(np.int64))       # out-degrees


def test_oracle_backward_against_torch_sparse_autograd(golden):
    """The BACKWARD of the operators, pinned by a library's own derivation: torch.sparse (`torch.sparse.mm`, `torch.sparse.softmax` and
    their autograd) computes the same aggregation and the same per-destination softmax on a sparse [dst, src] matrix without any of
    this repository's code.  oracle/ref_ops.py (autograd through index ops) and the C kernels' hand-written backward (oracle/c_ops.py)
    must give the same forward values AND the same gradients with respect to the node features, the edge weights and the edge logits.
    Simple graphs (torch coalesces duplicate entries; DGL's multigraph semantics are covered by the SciPy test above)."""
    from oracle import c_ops
    gen = torch.Generator().manual_seed(91)
    rs, rd = torch.randint(0, 60, (500,), generator=gen), torch.randint(0, 60, (500,), generator=gen)
    key = torch.unique(rs * 60 + rd)                                       # a random simple digraph with self-loops
    cases = [golden.graph("g64"), golden.graph("g300"), (key // 60, key % 60, 60)]
    for s, d, n in cases:
        assert torch.unique(s * n + d).numel() == s.numel()                # no parallel edges
        E, D = s.numel(), 6
        idx = torch.stack([d, s])                                          # row = destination, column = source
        x0 = torch.randn(n, D, generator=gen, dtype=torch.float64)
        w0 = torch.rand(E, generator=gen, dtype=torch.float64) + 0.1
        e0 = torch.randn(E, generator=gen, dtype=torch.float64) * 3
        gout = torch.randn(n, D, generator=gen, dtype=torch.float64)
        ga = torch.randn(E, generator=gen, dtype=torch.float64)

        def lib_side():
            x, w, e = (t.clone().requires_grad_() for t in (x0, w0, e0))
            out = torch.sparse.mm(torch.sparse_coo_tensor(idx, w, (n, n)), x)                       # u_mul_e_sum
            sm = torch.sparse.softmax(torch.sparse_coo_tensor(idx, e, (n, n)).coalesce(), dim=1)     # softmax over each destination's in-edges
            order = torch.argsort(d * n + s)                                                         # coalesced order -> edge order
            a = torch.empty_like(e0).index_put((order,), sm.values())
            ((out * gout).sum() + (a * ga).sum()).backward()
            return out.detach(), a.detach(), x.grad, w.grad, e.grad

        def oracle_side(dtype, ops_mod, graph):
            x, w, e = (t.clone().to(dtype).requires_grad_() for t in (x0, w0, e0))
            out = ops_mod.u_mul_e_sum(*graph, x.view(n, 1, D), w.view(E, 1, 1)).view(n, D)
            a = (ops_mod.edge_softmax(d, n, e.view(E, 1, 1)) if ops_mod is R else ops_mod.edge_softmax(graph[0], e.view(E, 1, 1))).view(E)
            ((out * gout.to(dtype)).sum() + (a * ga.to(dtype)).sum()).backward()
            return out.detach(), a.detach(), x.grad, w.grad, e.grad

        want = lib_side()
        got = oracle_side(torch.float64, R, (s, d, n))
        for g_, w_, name in zip(got, want, ("out", "a", "dx", "dw", "de")):
            np.testing.assert_allclose(g_.numpy(), w_.numpy(), rtol=1e-10, atol=1e-12, err_msg=f"ref_ops {name}")
        got = oracle_side(torch.float32, c_ops, (c_ops.CGraph(s, d, n),))
        for g_, w_, name in zip(got, want, ("out", "a", "dx", "dw", "de")):
            np.testing.assert_allclose(g_.double().numpy(), w_.numpy(), rtol=2e-4, atol=2e-5, err_msg=f"c_ops {name}")


def test_preprocess_edge_set_against_scipy(golden):
    """`preprocess` (run.py:133-148: to_bidirected, remove_self_loop, add_self_loop) as SET algebra done by SciPy: the edge set must be
    the symmetric closure of the raw edges without the diagonal, plus every self-loop exactly once — whatever the raw list holds
    (duplicates, self-loops, one-directional and already-bidirectional pairs).  The ORDER of the edges (DGL's convention: sorted pairs,
    self-loops appended last) is what the golden fixtures and the reference's call sites pin; this pins the set and the multiplicities."""
    import scipy.sparse as sp
    gen = torch.Generator().manual_seed(5)
    for n, e in ((1, 0), (7, 0), (40, 300), (300, 900), (64, 64 * 64)):
        s = torch.randint(0, n, (e,), generator=gen)
        d = torch.randint(0, n, (e,), generator=gen)
        ps, pd = R.preprocess_edges(s, d, n)
        A = sp.coo_matrix((np.ones(e), (s.numpy(), d.numpy())), shape=(n, n)).tocsr()
        S = ((A + A.T) != 0).astype(np.int64).tolil()
        S.setdiag(1)
        want = S.tocoo()
        got = sp.coo_matrix((np.ones(ps.numel()), (ps.numpy(), pd.numpy())), shape=(n, n)).tocsr()
        assert got.max() <= 1 if ps.numel() else True                               # no parallel edges
        assert ps.numel() == want.nnz
        assert (got != want.tocsr()).nnz == 0
        # self-loops come last, one per node in node order (run.py:146-147 `remove_self_loop().add_self_loop()`)
        assert torch.equal(ps[-n:], torch.arange(n)) and torch.equal(pd[-n:], torch.arange(n))
        assert bool((ps[:-n] != pd[:-n]).all())
