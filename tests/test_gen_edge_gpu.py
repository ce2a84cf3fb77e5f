"""DeeperGCN with raw edge features on the MI355X: the edge-feature softmax sweeps (csrc/spmm_softmax_edge.hip) entry for entry in their
three exact regimes (weight = 0: the unweighted sweeps' own results; beta = 0: the mean; beta = 128 with a unique maximum: that edge's
message and the routed gradients), under the derived bounds of tests/gen_edge_cases.py on seeded normal inputs (and against the tensor
form), their determinism, each gradient alone, the fall-back routes, non-finite inputs, and `GENConv(edge_dim=)`, `DeeperGCN(edge_dim=)`
and `workloads.build_gen_edge` end to end."""
import functools

import numpy as np
import pytest
import torch

from bot_amd import _C, ops, workloads
from bot_amd import nn as bnn
from bot_amd.sampling import MultiLayerNeighborSampler, NodeDataLoader
from tests import gen_edge_cases as GE
from tests.test_gen_gpu import _exp_error
from tests.test_sage_gpu import _block, _graphs, _parent, _same_bytes, _slab

pytestmark = pytest.mark.gpu
DEV = "cuda"
WIDTHS = (1, 4, 6, 7, 64, 250, 256, 516, 1000)     # 6: vec 2; 7: vec 1; 516: a second forward tile; 1000: four
KS = (1, 3, 8, 16)                                 # 8 and 16 read ef rows with 16-byte loads; 1 .. 4, 5 .. 8, 9 .. 16 are the three instances
BETAS = (0.1, 1.0, 10.0)
EPS = 1e-7
RATIOS = {}                                        # name -> the largest |error| / bound seen by the toleranced tests


def _beta(v):
    return torch.full((1,), float(v), dtype=torch.float32, device=DEV)


def _ratio(name, err, tol):
    """Records max(err / tol) under `name` and returns the entries over their bound."""
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(tol > 0, err / np.where(tol > 0, tol, 1.0), np.where(err > 0, np.inf, 0.0))
    RATIOS[name] = max(RATIOS.get(name, 0.0), float(r.max()) if r.size else 0.0)
    return np.argwhere(err > tol)


def _eperm(g):
    return ops._csc_edge_rows(g)


@functools.lru_cache(maxsize=None)
def _cases():
    """(name, graph, arrays): small_graph's sizes (isolated destinations, parallel edges, edge ids in no particular order; chunk = 4: long
    rows in both directions), a block-shaped graph, and a sampled block, whose edge id is its CSC position."""
    out = [(name, g) for name, g in _graphs()] + [("sampled", _block())]
    assert _eperm(out[-1][1]) is None and not np.array_equal(out[3][1].csc.eid.cpu().numpy(), np.arange(out[3][1].number_of_edges()))
    assert int((np.diff(out[3][1].csc.indptr.cpu().numpy()) == 0).sum()) >= 10
    return tuple((name, g, GE.arrays_of(g)) for name, g in out)


@functools.lru_cache(maxsize=None)
def _hub():
    from tests.test_subgraph_gpu import _hub_graph
    g = _hub_graph()
    assert int(np.diff(g.csc.indptr.cpu().numpy()).max()) > 2048 and g.csc.n_long > 0 and g.csr.n_long > 0
    return g, GE.arrays_of(g)


def _dev(a, pad=0):
    return None if a is None else (_slab(a, pad) if pad else torch.from_numpy(a).to(DEV))


def _forward(g, x, ef, w, b, beta, relu, eps, want_q, pad=0):
    return _C.spmm_softmax_edge(g.csc, _dev(x, pad), _dev(ef), _dev(w), _dev(b), _beta(beta), relu, eps, want_q, eperm=_eperm(g))


def _backward(g, x, ef, w, b, beta, relu, eps, dout, o, l, pad=0, **kw):
    return _C.spmm_softmax_edge_bwd(g.csr, _dev(x, pad), _dev(ef), _dev(w), _dev(b), _beta(beta), relu, eps, _dev(dout, pad), o, l,
                                    eperm=g.csr.eid, **kw)


def _ks(F_):
    return KS if F_ in (4, 7, 64, 256) else (8, KS[F_ % 4])


# ------------------------------------------------------------------------------------------------ 1. weight = 0: the unweighted sweeps
@pytest.mark.parametrize("F_", WIDTHS)
def test_zero_weight_gives_the_unweighted_sweeps_results(F_):
    """weight = 0 and no bias: z = x, so out, lse, q and dx are `_C.spmm_softmax` / `_C.spmm_softmax_bwd` on x, value for value (the two
    differ at most in the sign of a zero: 0 * ef is -0 for a negative ef)."""
    for name, g, _ in _cases():
        rng = np.random.default_rng(F_ + len(name))
        x = rng.standard_normal((g.number_of_src_nodes(), F_)).astype(np.float32)
        dout = rng.standard_normal((g.number_of_dst_nodes(), F_)).astype(np.float32)
        for K in KS:
            ef = rng.standard_normal((g.number_of_edges(), K)).astype(np.float32)
            w = np.zeros((F_, K), dtype=np.float32)
            for relu, beta, pad in ((False, 1.0, 0), (True, 1.0, 3), (True, 10.0, 4)):      # contiguous; an odd row stride; a strided slab
                o, l, q = _forward(g, x, ef, w, None, beta, relu, EPS, True, pad)
                o2, l2, q2 = _C.spmm_softmax(g.csc, _dev(x, pad), _beta(beta), relu, EPS, True)
                assert torch.equal(o, o2) and torch.equal(l, l2) and torch.equal(q, q2), (name, F_, K, relu)
                o3, l3, q3 = _forward(g, x, ef, w, None, beta, relu, EPS, False, pad)
                assert q3 is None and _same_bytes(o3, o) and _same_bytes(l3, l)
                dx, dw = _backward(g, x, ef, w, None, beta, relu, EPS, dout, o, l, pad)
                assert "spmm_softmax_edge_bwd_kernel<dw," in _C._lib.bot_last_kernel().decode()
                dx2 = _C.spmm_softmax_bwd(g.csr, _dev(x, pad), _beta(beta), relu, EPS, _dev(dout, pad), o2, l2)
                assert torch.equal(dx, dx2), (name, F_, K, relu)
                assert dw.shape == (F_, K) and bool(torch.isfinite(dw).all())


# ------------------------------------------------------------------------------------------------ 2. beta = 0: the mean
def _ints(rng, shape, lo, hi):
    return rng.integers(lo, hi + 1, shape).astype(np.float32)


@pytest.mark.parametrize("F_", WIDTHS)
def test_beta_zero_is_the_mean_bit_for_bit(F_):
    """beta = 0, eps = 0, integer-valued operands with every |z| and row sum below 2^24: every weight is exactly 1 and out =
    float32(sum of m) / float32(deg)."""
    for name, g, (src, dst, n_src, n_dst, indptr, eid) in _cases():
        rng = np.random.default_rng(7 * F_ + len(name))
        x = _ints(rng, (n_src, F_), -8, 8)
        for K in _ks(F_):
            ef, w, b = _ints(rng, (len(src), K), -3, 3), _ints(rng, (F_, K), -2, 2), _ints(rng, (F_,), -4, 4)
            z = x.astype(np.int64)[src] + ef.astype(np.int64) @ w.astype(np.int64).T + b.astype(np.int64)
            deg = np.bincount(dst, minlength=n_dst)
            for relu in (False, True):
                m = np.maximum(z, 0) if relu else z
                s = np.zeros((n_dst, F_), dtype=np.int64)
                np.add.at(s, dst, m)
                assert int(np.abs(z).max(initial=0)) < 2 ** 24 and int(np.abs(s).max(initial=0)) < 2 ** 24
                want = np.where(deg[:, None] > 0, s.astype(np.float32) / np.maximum(deg, 1).astype(np.float32)[:, None], np.float32(0))
                o, l, q = _forward(g, x, ef, w, b, 0.0, relu, 0.0, True, pad=3 if relu else 0)
                assert np.array_equal(o.cpu().numpy(), want.astype(np.float32)), (name, F_, K, relu)


# ------------------------------------------------------------------------------------------------ 3. beta = 128: the maximum
def _unique_max_inputs(arrays, F_, K, seed, relu):
    """Integer-valued operands with a unique maximal in-edge per (row, column), asserted here.  Column 0 of the weight is all ones, and in
    every row of two or more in-edges one edge's ef[., 0] is raised by 512, above the spread of z; a row of one in-edge keeps its z, of
    either sign, so under relu some winners are gated.  -> (x, ef, w, b, winner [n_dst, F] as an edge id or -1, z)."""
    src, dst, n_src, n_dst, indptr, eid = arrays
    rng = np.random.default_rng(seed)
    x, ef, w, b = _ints(rng, (n_src, F_), -8, 8), _ints(rng, (len(src), K), -3, 3), _ints(rng, (F_, K), -2, 2), _ints(rng, (F_,), -4, 4)
    w[:, 0] = 1
    deg = np.diff(indptr)
    for v in np.nonzero(deg >= 2)[0]:
        ef[eid[indptr[v] + rng.integers(0, deg[v])], 0] += 512
    z = x.astype(np.int64)[src] + ef.astype(np.int64) @ w.astype(np.int64).T + b.astype(np.int64)
    m = np.maximum(z, 0) if relu else z
    winner = np.full((n_dst, F_), -1, dtype=np.int64)
    for v in np.nonzero(deg >= 1)[0]:
        e = eid[indptr[v]:indptr[v + 1]]
        top = m[e].max(0)
        assert ((m[e] == top).sum(0) == 1).all(), "the maximum is not unique"
        winner[v] = e[np.argmax(m[e], axis=0)]
    assert int(np.abs(z).max(initial=0)) < 2 ** 20
    return x, ef, w, b, winner, z


@pytest.mark.parametrize("F_", WIDTHS)
def test_beta_128_routes_everything_to_the_unique_maximum(F_):
    cols = np.arange(F_)
    for name, g, arrays in _cases():
        src, dst, n_src, n_dst, indptr, eid = arrays
        for K in _ks(F_):
            for relu in (False, True):
                x, ef, w, b, winner, z = _unique_max_inputs(arrays, F_, K, 11 * F_ + K + len(name), relu)
                some = winner[:, 0] >= 0
                zw = np.where(some[:, None], z[np.maximum(winner, 0), cols[None, :]], 0)
                want = (np.maximum(zw, 0) if relu else zw).astype(np.float32)
                o, l, q = _forward(g, x, ef, w, b, 128.0, relu, 0.0, True)
                assert np.array_equal(o.cpu().numpy(), want), (name, F_, K, relu)
                assert np.array_equal(q.cpu().numpy(), want * want)
                dout = _ints(np.random.default_rng(F_ + K), (n_dst, F_), -8, 8)
                gate = some[:, None] & ((zw > 0) if relu else np.ones_like(zw, dtype=bool))
                if relu and name == "square65":
                    assert (~gate & some[:, None]).any()                        # some single-edge winners are gated
                routed = np.where(gate, dout.astype(np.int64), 0)
                want_dx, want_dw = np.zeros((n_src, F_), dtype=np.int64), np.zeros((F_, K), dtype=np.int64)
                vv, ff = np.nonzero(gate)
                np.add.at(want_dx, (src[winner[vv, ff]], ff), routed[vv, ff])
                np.add.at(want_dw, ff, routed[vv, ff][:, None] * ef.astype(np.int64)[winner[vv, ff]])
                dx, dw = _backward(g, x, ef, w, b, 128.0, relu, 0.0, dout, o, l)
                assert np.array_equal(dx.cpu().numpy(), want_dx.astype(np.float32)), (name, F_, K, relu)
                assert np.array_equal(dw.cpu().numpy(), want_dw.astype(np.float32)), (name, F_, K, relu)


# ------------------------------------------------------------------------------------------------ 4. normal inputs under the derived bounds
def _normal(arrays, F_, K, seed, bias=True):
    src, dst, n_src, n_dst, _, _ = arrays
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n_src, F_)).astype(np.float32)
    ef = rng.standard_normal((len(src), K)).astype(np.float32)
    w = (rng.standard_normal((F_, K)) / np.sqrt(K)).astype(np.float32)
    b = rng.standard_normal(F_).astype(np.float32) if bias else None
    dout = rng.standard_normal((n_dst, F_)).astype(np.float32)
    return x, ef, w, b, dout


def _check_normal(name, g, arrays, F_, K, beta, relu, seed, bias=True, pad=0, tensor_form=True):
    x, ef, w, b, dout = _normal(arrays, F_, K, seed, bias)
    exp_err = _exp_error()
    res = GE.forward64(arrays, x, ef, w, b, beta, relu, EPS)
    tol = GE.forward_bounds(res, beta, exp_err)
    o, l, q = _forward(g, x, ef, w, b, beta, relu, EPS, True, pad)
    for key, got in (("out", o), ("lse", l), ("q", q)):
        over = _ratio(f"forward {key}", np.abs(got.cpu().double().numpy() - res[key]), tol[key])
        assert over.size == 0, (name, F_, K, beta, relu, key, over[:3])
    empty = res["deg"] == 0
    assert not o.cpu().numpy()[empty].any() and not l.cpu().numpy()[empty].any() and not q.cpu().numpy()[empty].any()
    grads, gtol = GE.backward64(arrays, x, ef, w, b, beta, relu, EPS, dout, o.cpu().numpy(), l.cpu().numpy(), exp_err)
    dx, dw = _backward(g, x, ef, w, b, beta, relu, EPS, dout, o, l, pad)
    for key, got in (("dx", dx), ("dweight", dw)):
        over = _ratio(f"backward {key}", np.abs(got.cpu().double().numpy() - grads[key]), gtol[key])
        assert over.size == 0, (name, F_, K, beta, relu, key, over[:3])
    if not tensor_form:
        return
    # the op, kernel form against tensor form: both are held to the bounds, so they differ by at most their sum
    leaves = lambda: [torch.from_numpy(t).to(DEV).requires_grad_() for t in ((x, w, b) if bias else (x, w))]
    outs = {}
    for impl in ("kernel", "tensor"):
        lv = leaves()
        bt = _beta(beta).requires_grad_()
        out = ops.u_add_e_softmax(g, lv[0], _dev(ef), lv[1], lv[2] if bias else None, bt, relu=relu, eps=EPS, impl=impl)
        out.backward(_dev(dout))
        outs[impl] = [out.detach()] + [t.grad for t in lv] + [bt.grad]
    dxc, dwc = _backward(g, x, ef, w, b, beta, relu, EPS, dout, o, l)      # contiguous operands, as the op passes them: the lane groups, and
    assert _same_bytes(dxc, dx)                                            # with them the order of dweight's fold, follow the vector width
    assert _same_bytes(outs["kernel"][0], o) and _same_bytes(outs["kernel"][1], dx) and _same_bytes(outs["kernel"][2], dwc)
    _, ttol = GE.backward64(arrays, x, ef, w, b, beta, relu, EPS, dout, o.cpu().numpy(), l.cpu().numpy(), exp_err, own_forward=tol)
    over = _ratio("kernel form - tensor form, out", (outs["kernel"][0] - outs["tensor"][0]).abs().cpu().double().numpy(), 2.0 * tol["out"])
    assert over.size == 0, (name, F_, K, beta, relu)
    for i, key in ((1, "dx"), (2, "dweight")) + (((3, "dbias"),) if bias else ()):
        k64, t64 = outs["kernel"][i].cpu().double().numpy(), outs["tensor"][i].cpu().double().numpy()
        assert _ratio(f"op {key}", np.abs(k64 - grads[key]), gtol[key]).size == 0, (name, F_, K, beta, relu, key)
        # the sum of the two bounds; the tensor form's gradient runs through its own float32 out and lse (own_forward)
        assert _ratio(f"kernel form - tensor form, {key}", np.abs(k64 - t64), gtol[key] + ttol[key]).size == 0, (name, F_, K, beta, relu, key)
    dbeta = GE.dbeta64(res, dout)
    btol = GE.dbeta_bound(res, tol, dout)
    got = float(outs["kernel"][-1])
    RATIOS["op dbeta"] = max(RATIOS.get("op dbeta", 0.0), abs(got - dbeta) / btol)
    assert abs(got - dbeta) <= btol, (name, F_, K, beta, relu, got, dbeta, btol)


@pytest.mark.parametrize("F_", WIDTHS)
def test_normal_inputs_under_the_derived_bounds(F_):
    i = 0
    for name, g, arrays in _cases():
        if name in ("square1", "square63", "square64") and F_ not in (4, 64):
            continue                                      # the other five graphs at every width; these three at two
        for K in _ks(F_):
            beta, relu = BETAS[i % 3], bool((i // 3 + i) % 2)
            i += 1
            _check_normal(name, g, arrays, F_, K, beta, relu, 13 * F_ + K, bias=i % 4 != 0, pad=(0, 3, 4)[i % 3])


@pytest.mark.parametrize("beta", BETAS)
@pytest.mark.parametrize("relu", [False, True])
def test_normal_inputs_every_beta_and_gate(beta, relu):
    for name, g, arrays in _cases()[3:]:
        _check_normal(name, g, arrays, 64, 8, beta, relu, 5)
        _check_normal(name, g, arrays, 7, 3, beta, relu, 6)


def test_normal_inputs_on_the_hub_graph():
    """Rows above 2 048 in-edges and out-edges: the chunks, both combines, and more than one stride of the persistent loop."""
    g, arrays = _hub()
    _check_normal("hub", g, arrays, 4, 3, 1.0, True, 3, tensor_form=False)
    _check_normal("hub", g, arrays, 5, 8, 10.0, False, 4, tensor_form=False)


# ------------------------------------------------------------------------------------------------ 5. determinism, each gradient alone
@pytest.mark.parametrize("F_,K", [(256, 8), (64, 16), (8, 3), (1000, 8)])
def test_two_calls_give_the_same_bytes(F_, K):
    g, arrays = _hub()                                    # 30 000 rows: the backward's workgroups each stride more than once at F = 256
    assert g.csr.n_items > 16 * 1024
    x, ef, w, b, dout = _normal(arrays, F_, K, 1)
    runs = []
    for _ in range(2):
        o, l, q = _forward(g, x, ef, w, b, 1.0, True, EPS, True)
        dx, dw = _backward(g, x, ef, w, b, 1.0, True, EPS, dout, o, l)
        runs.append((o, l, q, dx, dw))
    assert all(_same_bytes(a, c) for a, c in zip(*runs))
    assert bool(torch.isfinite(runs[0][4]).all()) and float(runs[0][4].abs().max()) > 0
    # one gradient at a time: the same bytes as together (the instance without dweight carries no partials; dx is the same arithmetic)
    o, l = runs[0][0], runs[0][1]
    dx1, none = _backward(g, x, ef, w, b, 1.0, True, EPS, dout, o, l, want_dweight=False)
    assert none is None and _same_bytes(dx1, runs[0][3])
    assert "spmm_softmax_edge_bwd_kernel<" in _C._lib.bot_last_kernel().decode() and "<dw," not in _C._lib.bot_last_kernel().decode()
    none, dw1 = _backward(g, x, ef, w, b, 1.0, True, EPS, dout, o, l, want_dx=False)
    assert none is None and _same_bytes(dw1, runs[0][4])
    for name, g2, arr2 in _cases()[4:6]:
        x, ef, w, b, dout = _normal(arr2, F_, K, 2)
        a = _forward(g2, x, ef, w, b, 1.0, True, EPS, True)
        c = _forward(g2, x, ef, w, b, 1.0, True, EPS, True)
        assert all(_same_bytes(s, t) for s, t in zip(a, c))
        assert all(_same_bytes(s, t) for s, t in zip(_backward(g2, x, ef, w, b, 1.0, True, EPS, dout, a[0], a[1]),
                                                     _backward(g2, x, ef, w, b, 1.0, True, EPS, dout, a[0], a[1])))


def test_each_gradient_alone_matches_all_at_once():
    name, g, arrays = _cases()[4]
    x, ef, w, b, dout = _normal(arrays, 40, 8, 9)

    def run(need):
        lv = [torch.from_numpy(t).to(DEV).requires_grad_(k in need) for k, t in (("x", x), ("weight", w), ("bias", b))]
        bt = _beta(0.7).requires_grad_("beta" in need)
        ops.u_add_e_softmax(g, lv[0], _dev(ef), lv[1], lv[2], bt, relu=True, eps=EPS).backward(_dev(dout))
        return dict(zip(("x", "weight", "bias", "beta"), [t.grad for t in lv] + [bt.grad]))
    both = run(("x", "weight", "bias", "beta"))
    assert all(v is not None for v in both.values())
    for key in both:
        alone = run((key,))
        assert all((v is None) == (k != key) for k, v in alone.items())
        assert _same_bytes(alone[key], both[key]), key
    assert _same_bytes(both["bias"], torch.sum(both["x"], dim=0, dtype=torch.float64).float())       # dbias = the column sum of dx


# ------------------------------------------------------------------------------------------------ 6. routes
def test_wide_and_differentiated_edge_features_run_the_tensor_form():
    name, g, arrays = _cases()[3]
    calls = []
    real = _C.spmm_softmax_edge
    _C.spmm_softmax_edge = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        x, ef, w, b, dout = _normal(arrays, 12, 17, 3)
        res = GE.forward64(arrays, x, ef, w, b, 1.0, True, EPS)
        tol = GE.forward_bounds(res, 1.0, _exp_error())
        out = ops.u_add_e_softmax(g, _dev(x), _dev(ef), _dev(w), _dev(b), 1.0, relu=True, eps=EPS)            # K = 17
        assert calls == [] and _ratio("tensor form, K = 17", np.abs(out.cpu().double().numpy() - res["out"]), tol["out"]).size == 0
        x, ef, w, b, dout = _normal(arrays, 12, 8, 4)
        res = GE.forward64(arrays, x, ef, w, b, 1.0, True, EPS)
        tol = GE.forward_bounds(res, 1.0, _exp_error())
        efd = _dev(ef).requires_grad_()
        out = ops.u_add_e_softmax(g, _dev(x), efd, _dev(w), _dev(b), 1.0, relu=True, eps=EPS)                # ef asks for a gradient
        out.backward(_dev(dout))
        assert calls == [] and efd.grad is not None
        assert _ratio("tensor form, ef.requires_grad", np.abs(out.detach().cpu().double().numpy() - res["out"]), tol["out"]).size == 0
        with torch.no_grad():
            ops.u_add_e_softmax(g, _dev(x), efd, _dev(w), _dev(b), 1.0, relu=True, eps=EPS)                  # no gradient can be asked for
        assert calls == [1]
    finally:
        _C.spmm_softmax_edge = real
    with pytest.raises(_C.BotKernelError, match="K <= 16"):
        _C.spmm_softmax_edge(g.csc, _dev(x), torch.zeros(g.number_of_edges(), 17, device=DEV), torch.zeros(12, 17, device=DEV), None, _beta(1.0))


POISON_X, POISON_E = [50], [105]      # one source row and one edge of the long-row graph: they reach two destinations and five sources


def test_nan_stays_inside_the_rows_that_gather_it():
    name, g, (src, dst, n_src, n_dst, indptr, eid) = _cases()[4]              # long rows: the chunks and both combines
    x, ef, w, b, dout = _normal((src, dst, n_src, n_dst, indptr, eid), 12, 8, 1)
    bad_x = np.zeros(n_src, dtype=bool)
    bad_x[POISON_X] = True
    bad_e = np.zeros(len(src), dtype=bool)
    bad_e[POISON_E] = True
    px, pe = x.copy(), ef.copy()
    px[bad_x, ::2] = np.nan
    pe[bad_e, 3] = np.nan
    hit_dst = np.zeros(n_dst, dtype=bool)
    hit_dst[dst[bad_x[src] | bad_e]] = True
    hit_src = bad_x.copy()
    hit_src[src[hit_dst[dst]]] = True
    assert 2 <= hit_dst.sum() <= n_dst - 10 and hit_src.sum() <= n_src - 5
    for relu in (False, True):
        runs = []
        for xv, ev in ((px, pe), (np.where(np.isnan(px), np.float32(0), px), np.where(np.isnan(pe), np.float32(0), pe))):
            o, l, q = _forward(g, xv, ev, w, b, 1.0, relu, EPS, True)
            dx, _ = _backward(g, xv, ev, w, b, 1.0, relu, EPS, dout, o, l)
            runs.append([t.cpu().numpy() for t in (o, l, q, dx)])
        for k in range(3):
            assert np.array_equal(runs[0][k][~hit_dst], runs[1][k][~hit_dst]) and np.isfinite(runs[0][k][~hit_dst]).all()
            assert np.isnan(runs[0][k][hit_dst]).any()
        assert np.array_equal(runs[0][3][~hit_src], runs[1][3][~hit_src]) and np.isfinite(runs[0][3][~hit_src]).all()


# ------------------------------------------------------------------------------------------------ 7. GENConv, DeeperGCN, the recipe
@pytest.mark.parametrize("kw", [dict(), dict(learn_beta=True, beta=0.5, msg_norm=True, learn_msg_scale=True, mlp_layers=2)])
@pytest.mark.parametrize("fin,fout", [(3, 16), (41, 16)])
def test_genconv_edge_dim_against_fp64_restatement(kw, fin, fout):
    calls = []
    real = _C.spmm_softmax_edge
    _C.spmm_softmax_edge = lambda *a, **k: calls.append(1) or real(*a, **k)
    try:
        GE.check_conv(_parent(), DEV, fin, fout, 8, **kw)
    finally:
        _C.spmm_softmax_edge = real
    assert calls == [1]                                                       # the layer runs the kernel form
    GE.check_conv(_block(), DEV, fin, fout, 8, seed=1, **kw)
    g = _parent()
    sub = g.subgraph(torch.randperm(g.number_of_nodes(), generator=torch.Generator().manual_seed(4))[:1500])
    GE.check_conv(sub, DEV, fin, fout, 8, seed=2, **kw)
    GE.check_conv(_graphs()[3][1], DEV, fin, fout, 8, seed=3, **kw)           # isolated destinations


@pytest.mark.parametrize("kw", [dict(), dict(learn_beta=True, msg_norm=True, mlp_layers=2, beta=0.5)])
def test_deepergcn_edge_dim_against_fp64_restatement(kw):
    from tests import block_cases as BC
    g = BC.parent_graph(DEV, n=3000, e_raw=22000)
    ef = torch.rand(g.number_of_edges(), 8, generator=torch.Generator().manual_seed(6))
    g.edata["feat"] = ef.to(DEV)
    torch.manual_seed(3)
    GE.check_stack(bnn.DeeperGCN(8, 5, 12, 3, dropout=0.5, edge_dim=8, **kw), g, g.ndata["feat"].cpu(), ef, DEV)
    nids = torch.randperm(3000, generator=torch.Generator().manual_seed(3))[:600]
    _, _, blocks = next(iter(NodeDataLoader(g, nids, MultiLayerNeighborSampler([5, 7, 9]), batch_size=600, seed=4)))
    per_block = [b.edata["feat"].cpu() for b in blocks]
    model = bnn.DeeperGCN(8, 5, 12, 3, edge_dim=8, **kw)
    GE.check_stack(model, blocks, blocks[0].srcdata["feat"].cpu(), per_block, DEV)
    with torch.no_grad():                                                     # None: each block's rows of the parent's column
        assert torch.equal(model(blocks), model(blocks, None, [e.to(DEV) for e in per_block]))


def test_build_gen_edge_full_batch_step():
    wl = workloads.build_gen_edge("proteins", DEV, scale=0.02)
    loss, pred = wl.step()
    assert np.isfinite(float(loss.detach())) and pred.shape == (wl.n_nodes, 112)
    assert "spmm_softmax_edge" in wl.dominant[0]
    params = dict(wl.model.named_parameters())
    assert "convs.1.beta" in params and "convs.2.lin_edge.weight" in params
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params.values())
    loss2, _ = wl.step()
    assert np.isfinite(float(loss2.detach()))


def test_build_gen_edge_sampled_epoch():
    wl = workloads.build_gen_edge("proteins", DEV, sampled=True, scale=0.02)
    assert len(wl.loader) == workloads.SAMPLED["proteins"][1] and wl.evaluator is not None
    loss = wl.epoch()
    assert np.isfinite(float(loss))
    params = dict(wl.model.named_parameters())
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in params.values())
    assert params["convs.0.lin_edge.weight"].grad is not None


def test_report_measured_figures():
    """Prints what the README section quotes (run after the tests above in file order; it asserts what they asserted: no ratio above 1)."""
    for k, v in sorted(RATIOS.items()):
        print(f"largest error / bound, {k}: {v:.4f}")
    assert all(v <= 1.0 for v in RATIOS.values())
