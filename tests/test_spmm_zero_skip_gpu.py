"""The zero-weight skip of the weighted sweeps (csrc/spmm.hip, `_C.spmm_set_zero_skip`) on the MI355X: with the switch on, an (edge, head)
whose weight is exactly 0 issues no loads of that head's part of the neighbour row.  Held to the switch-off arithmetic bit for bit on finite
data, to a float64 reference at the tolerances of tests/test_gpu_parity.py, and shown to really leave the rows unread (NaN slabs behind
zero weights reach the results only with the switch off).

One direction of ~600 rows: degrees 0, 1, 3, 4, 5, 63, 64, 65, one row longer than two default chunks (partial / combine path), the
rest short.  Shapes (3, 250) = the benchmark's instantiation (a head spans two whole waves), (2, 200) a head per wave, (3, 40) four heads
per wave (per-lane predicate), (1, 40) the output layer's head-major kernels."""
import pytest
import torch

import bot_amd
from bot_amd import _C, gemm
from bot_amd import nn as bnn
from bot_amd.nn import fused

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 600
SHAPES = ((3, 250), (2, 200), (3, 40), (1, 40))
SPECIAL = (0, 1, 3, 4, 5, 63, 64, 65)     # degrees of rows 0 .. 7; row 8 is the long one


@pytest.fixture(autouse=True)
def _switch_back_on():
    yield
    _C.spmm_set_zero_skip(1)


class Case:
    pass


_CASES = {}


def _case(H, D):
    """Structure, operands, weights and float64 references of one shape, built once."""
    if (H, D) in _CASES:
        return _CASES[(H, D)]
    gen = torch.Generator().manual_seed(100 * H + D)
    deg = torch.randint(1, 13, (N,), generator=gen)
    deg[:len(SPECIAL)] = torch.tensor(SPECIAL)
    chunk = _C.default_chunk(int(deg.sum()) + 2000)
    deg[8] = 2 * chunk + 5
    rows = torch.repeat_interleave(torch.arange(N), deg)
    E = int(rows.numel())
    cols = torch.randint(0, N, (E,), generator=gen)
    # the direction under test is the CSR of this graph (rows = sources): w lives in CSC position order, reached through csr2csc
    g = bot_amd.Graph(rows, cols, N).to(DEV)
    d, wperm = g.csr, g.csr2csc
    assert d.chunk == _C.default_chunk(E) and d.n_long == 2 and int(deg[8]) > 2 * d.chunk   # (the row of 65 is long too: 64 + 1)
    c = Case()
    c.H, c.D, c.E, c.g, c.d, c.wperm = H, D, E, g, d, wperm
    indptr, idx = d.indptr.long(), d.indices.long()
    c.row_of = torch.repeat_interleave(torch.arange(N, device=DEV), indptr[1:] - indptr[:-1])
    c.idx = idx
    # weights in the direction's position order, then scattered to where wperm finds them
    wk = torch.randn(E, H, generator=gen)
    wk[torch.rand(E, H, generator=gen) < 0.3] = 0.0
    wk = wk.to(DEV)
    beg = lambda r: int(indptr[r])
    wk[beg(4):beg(5)] = 0.0                              # a row with every edge dropped
    wk[beg(6) + 10] = 0.0                                # an edge with every head dropped
    wk[beg(7) + 3] = 0.0                                 # the last edge of a group of four
    wk[beg(7) + 64, H - 1] = 0.0                         # ... and the lone edge of the row's second batch, one head
    wk[beg(8) + d.chunk: beg(8) + 2 * d.chunk] = 0.0     # a whole chunk of the long row
    cold_head, cold_all = torch.arange(20, 50, device=DEV), torch.arange(50, 70, device=DEV)
    wk[torch.isin(idx, cold_head), H - 1] = 0.0          # sources whose last head is reached through zero weights only
    wk[torch.isin(idx, cold_all)] = 0.0                  # ... and sources no head of which is wanted
    assert abs(float((wk == 0).float().mean()) - 0.35) < 0.1
    c.wk = wk
    c.w = torch.empty_like(wk)
    c.w[wperm.long()] = wk
    c.x = torch.randn(N, H, D, generator=gen).to(DEV)
    c.y = torch.randn(N, H, D, generator=gen).to(DEV)
    c.addend = torch.randn(N, H, D, generator=gen).to(DEV)
    # head slabs of x that only zero weights reach (a source that no edge names counts)
    hits = torch.zeros(N, H, device=DEV).index_add_(0, idx, (wk != 0).float())
    c.unread = hits == 0
    named = torch.zeros(N, device=DEV).index_add_(0, idx, torch.ones(E, device=DEV)) > 0
    assert int((c.unread & named[:, None]).sum()) >= 50
    c.x_nan = c.x.clone()
    c.x_nan[c.unread] = float("nan")
    c.hit_nan = c.unread[idx]                            # [E, H]: the entry gathers a NaN slab
    c.row_nan = torch.zeros(N, H, device=DEV).index_add_(0, c.row_of, c.hit_nan.float()) > 0
    assert c.row_nan.any() and not c.row_nan.all()
    x64 = c.x.double()
    c.ref_out = torch.zeros(N, H, D, dtype=torch.float64, device=DEV).index_add_(0, c.row_of, wk.double()[:, :, None] * x64[idx])
    ref_dot_k = (c.y.double()[c.row_of] * x64[idx]).sum(2)
    c.ref_dot = torch.empty_like(ref_dot_k)
    c.ref_dot[wperm.long()] = ref_dot_k
    _CASES[(H, D)] = c
    return c


def _halves_buf(c):
    return torch.zeros(N, 2 * c.H * c.D, dtype=torch.float16, device=DEV)


def _run(c, on, x):
    """Every entry point under one setting of the switch: (kernel name, result) per entry."""
    _C.spmm_set_zero_skip(on)
    H, D = c.H, c.D
    res = {}
    res["spmm"] = _C.spmm(c.d, x, c.w, c.wperm)
    res["spmm_kernel"] = _C._lib.bot_last_kernel().decode()
    res["spmm_addend"] = _C.spmm(c.d, x, c.w, c.wperm, addend=c.addend)
    res["spmm_pos"] = _C.spmm(c.d, x, c.wk)             # weights in position order, no wperm: the forward sweep of a layer
    out, dot = _C.spmm_dot(c.d, x, c.w, c.wperm, c.y)
    res["dot_out"], res["dot"] = out, dot
    res["dot_kernel"] = _C._lib.bot_last_kernel().decode()
    if H >= 2:
        buf = _halves_buf(c)
        assert _C.spmm_dot_halves_fits(x, c.y, buf, D, H * D)
        res["halves_dot"] = _C.spmm_dot_halves(c.d, x, c.w, c.wperm, c.y, torch.ones(1, device=DEV), buf, D, H * D)
        res["halves"] = buf
    torch.cuda.synchronize()
    return res


_RUNS = {}


def _runs(H, D):
    if (H, D) not in _RUNS:
        c = _case(H, D)
        _RUNS[(H, D)] = (_run(c, 0, c.x), _run(c, 1, c.x))
    return _RUNS[(H, D)]


def _halves_value(buf, H, D):
    return (buf[:, :H * D].double() + buf[:, H * D:].double() / 2048.0).unflatten(1, (H, D))


def test_kernels_under_test():
    """The shapes reach the kernels they are meant to (the benchmark's instantiation among them)."""
    names = {hd: (_runs(*hd)[1]["spmm_kernel"], _runs(*hd)[1]["dot_kernel"]) for hd in SHAPES}
    assert names[(3, 250)] == ("bot::spmm_rows_kernel<2,64,6,2>", "bot::spmm_dot_rows_kernel<2,64,6,2>")
    assert names[(2, 200)] == ("bot::spmm_rows_kernel<4,64,2,1>", "bot::spmm_dot_rows_kernel<4,64,2,1>")
    assert names[(3, 40)] == ("bot::spmm_rows_kernel<4,16,1,1>", "bot::spmm_dot_rows_kernel<4,16,1,1>")
    assert names[(1, 40)] == ("bot::spmm_kernel<4,16,1,true>", "bot::spmm_dot_kernel<4,16,1>")


@pytest.mark.parametrize("H,D", SHAPES)
def test_on_equals_off_bitwise(H, D):
    c = _case(H, D)
    off, on = _runs(H, D)
    nz = c.w != 0
    for key in ("spmm", "spmm_addend", "spmm_pos", "dot_out") + (("halves",) if H >= 2 else ()):
        assert torch.equal(off[key], on[key]), key
    for key in ("dot",) + (("halves_dot",) if H >= 2 else ()):
        assert torch.equal(off[key][nz], on[key][nz]), key
        assert bool((on[key][~nz] == 0).all()), f"{key}: entries of zero weights must be 0.f with the switch on"
        assert float(off[key][~nz].abs().max()) > 0          # (off computes them: the two settings do differ there)


@pytest.mark.parametrize("H,D", SHAPES)
def test_against_float64(H, D):
    c = _case(H, D)
    nz = c.w != 0
    close = lambda got, ref, atol: torch.testing.assert_close(got.double(), ref, atol=atol, rtol=1e-4)
    for on, res in enumerate(_runs(H, D)):
        close(res["spmm"], c.ref_out, 1e-4)
        close(res["spmm_pos"], c.ref_out, 1e-4)
        close(res["spmm_addend"], c.ref_out + c.addend.double(), 1e-4)
        close(res["dot_out"], c.ref_out, 1e-4)
        ref_dot = torch.where(nz, c.ref_dot, torch.zeros_like(c.ref_dot)) if on else c.ref_dot
        close(res["dot"], ref_dot, 1e-3 * D ** 0.5)
        if H >= 2:
            close(res["halves_dot"], ref_dot, 1e-3 * D ** 0.5)
            close(_halves_value(res["halves"], H, D), c.ref_out, 1e-4)


@pytest.mark.parametrize("H,D", SHAPES)
def test_zero_weight_rows_are_not_read(H, D):
    """NaN in every head slab that only zero weights reach: invisible with the switch on, everywhere it is gathered with it off."""
    c = _case(H, D)
    clean = _runs(H, D)[1]
    on = _run(c, 1, c.x_nan)
    for key in ("spmm", "spmm_addend", "spmm_pos", "dot_out", "dot") + (("halves", "halves_dot") if H >= 2 else ()):
        assert bool(torch.isfinite(on[key].float()).all()), key
        assert torch.equal(on[key], clean[key]), key     # = the float64 reference with those slabs zeroed (test_against_float64)
    off = _run(c, 0, c.x_nan)
    bad = c.row_nan[:, :, None].expand(N, H, D)
    for key in ("spmm", "spmm_addend", "spmm_pos", "dot_out"):
        assert bool(torch.isnan(off[key][bad]).all()) and bool(torch.isfinite(off[key][~bad]).all()), key
    hit = torch.zeros_like(c.hit_nan)
    hit[c.wperm.long()] = c.hit_nan
    assert bool(torch.isnan(off["dot"][hit]).all()) and bool(torch.isfinite(off["dot"][~hit]).all())
    if H >= 2:
        assert bool(torch.isnan(off["halves_dot"][hit]).all())
        assert bool(torch.isnan(_halves_value(off["halves"], H, D)[bad]).all())


@pytest.mark.parametrize("H,D", ((3, 250), (3, 40)))
def test_gat_hidden_layer_bitwise(H, D):
    """One fused GAT hidden layer, attention dropout 0.5, forward and backward under the same seeds: the output and every gradient
    are the same bit for bit with the switch on and off."""
    c = _case(H, D)
    g = c.g.add_self_loop().to(DEV)
    fin = H * D
    torch.manual_seed(5)
    conv = bnn.GATConv(fin, D, num_heads=H, attn_drop=0.5, linear=True, non_interactive_attn=True).to(DEV)
    bn = torch.nn.BatchNorm1d(H * D).to(DEV)
    h0 = torch.randn(N, fin, device=DEV)
    gout = torch.randn(N, H * D, device=DEV)
    assert not fused.use_agg_first(conv)
    min_rows, res = gemm.MIN_ROWS, []
    gemm.MIN_ROWS = 256                                  # the halves GEMMs, and with them the halves form of the backward sweep, at this size
    try:
        for on in (0, 1):
            _C.spmm_set_zero_skip(on)
            torch.manual_seed(17)
            h = h0.clone().requires_grad_()
            params = [h] + list(conv.parameters()) + list(bn.parameters())
            for p in params:
                p.grad = None
            bn.reset_running_stats()
            y = fused.gat_hidden_layer(conv, bn, g, h, 0.5, True)
            (y * gout).sum().backward()
            torch.cuda.synchronize()
            res.append([y.detach().clone()] + [p.grad.clone() for p in params])
    finally:
        gemm.MIN_ROWS = min_rows
    assert len(res[0]) == len(res[1]) >= 6
    for a, b in zip(*res):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b)
    assert float(res[0][0].abs().max()) > 0 and float(res[0][1].abs().max()) > 0
