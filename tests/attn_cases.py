"""Float64 restatements of the GAT attention and segment-sum contracts (include/bot_gnn.h bot_gat_attn_fwd_f32, bot_gat_attn_bwd_f32,
bot_segment_sum_f32; the docstrings of bot_amd/_C.py), shared by tests/test_attn_host.py and tests/test_attn_gpu.py: the forward with
its zsign byte, the backward, the segment sum and the Philox attention-dropout mask; the graphs of the row classes; the input builders
of the exact regimes, with their conditions ASSERTED while the inputs are built; and the bound functions for seeded inputs, built only
from lengths and magnitudes of the restatement.  Nothing here calls the code under test.

The kernel (csrc/attn.hip): lanes run across the edges of a row, a 16-lane group per short row and a 256-thread workgroup per long row
(in-degree above the row plan's chunk), so one lane walks L = ceil(deg / 16) or ceil(deg / 256) edges with an online softmax (running
max m, running sum s = s expf(m - m') + expf(e - m')); the lanes are combined with one more expf(m - M) each, and the second pass writes
expf(e - M) * (1 / sum).  Heads are held in registers in tiles of up to 8.

`EXPF_ERR`: the relative error of the device library's expf.  Measured on the MI355X (tests/test_attn_gpu.py
test_expf_error_measured_fp64) against float64 exp on two-edge rows with logits (0, t): the ratio of the two weights is expf(t) up to
the 2 U of the two products by 1 / sum.  On 3 000 seeded float32 t in [-87, 0] (results that are normal float32 numbers) the largest
relative error of the ratio was EXPF_MEASURED; the constant is twice that, as tests/dot_attn_cases.EXP_ERR was taken.  Below -87.3 the
result is a subnormal number and no relative error can be stated (the format itself holds fewer bits there): those weights are below
2^-126 of the row's largest and are held by the absolute term TINY of the bound instead."""
import functools

import numpy as np
import torch

from tests import sage_cases as SG
from tests.test_sampling_host import M64, philox4x32_10

F64 = torch.float64
U = 2.0 ** -24                 # the unit roundoff of float32
EXACT_LIMIT = 2.0 ** 22        # sums of multiples of 0.25 whose absolute terms add up to less than this are exact in float32
EXPF_MEASURED = 1.122e-07      # 1.1219e-07 = 1.882 U seen, at t = -0.5856154561042786 (below the 4 U above which it would be a finding)
EXPF_ERR = 2 * EXPF_MEASURED   # 2.244e-07
TINY = 2.0 ** -120             # absolute slack of a weight: subnormal exponentials (below 2^-126, times at most 2^6 terms of a lane)
GOLDEN = 0x9E3779B97F4A7C15
HEADS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 16, 17)
SUBSETS = (("el",), ("er",), ("ee",), ("el", "er"), ("el", "ee"), ("er", "ee"), ("el", "er", "ee"))
kRowLanes, kBlock = 16, 256


# ------------------------------------------------------------------------------------------------ graphs
def lanes_edges(seed=5):
    """(src, dst, n_src, n_dst) of the "lanes" graph: 24 destinations whose in-degrees include 0, 1, 15, 16, 17, 33 (one lane, then two
    and three edges per lane of a 16-lane group) and 255, 256, 257 (the 256-thread workgroup's stride, when the chunk makes them long
    rows); 64 sources drawn with replacement, edge ids in no particular order."""
    rng = np.random.default_rng(seed)
    deg = np.array([3, 0, 1, 15, 16, 17, 33, 255, 256, 257, 2, 0, 7, 16, 1, 12, 5, 9, 0, 4, 8, 2, 6, 11])
    dst = np.repeat(np.arange(deg.size), deg)
    src = rng.integers(0, 64, dst.size)
    order = rng.permutation(dst.size)
    return torch.from_numpy(src[order]), torch.from_numpy(dst[order]), 64, int(deg.size)


def _lanes(chunk):
    import bot_amd
    src, dst, n_src, n_dst = lanes_edges()
    return bot_amd.Graph(src, dst, n_src, num_dst_nodes=n_dst, chunk=chunk)


def _sweep(chunk):
    import bot_amd
    src, dst, n = SG.sweep_edges()
    return bot_amd.Graph(src, dst, n, chunk=chunk)


def graph_specs():
    """(name, builder of the CPU graph, number of long CSC rows or None for "some").  No graph has more than 3 000 edges."""
    out = [("sweep8", functools.partial(_sweep, 8), None), ("sweep128", functools.partial(_sweep, 128), 0),
           ("lanes300", functools.partial(_lanes, 300), 0), ("lanes16", functools.partial(_lanes, 16), 5)]
    for n in (1, 15, 16, 17):
        out.append((f"square{n}", functools.partial(SG.small_graph, n, n, 20 + n, chunk=300), 0))
        out.append((f"square{n}long", functools.partial(SG.small_graph, n, n, 20 + n, chunk=4), None))
    out.append(("block", functools.partial(SG.small_graph, 17, 50, 31, chunk=300), 0))
    out.append(("blocklong", functools.partial(SG.small_graph, 33, 70, 32, chunk=4), None))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def graphs():
    """The CPU graphs, built once, with their row classes asserted."""
    out = []
    for name, make, n_long in graph_specs():
        g = make()
        assert g.number_of_edges() <= 3000
        assert (g.csc.n_long > 0) if n_long is None else (g.csc.n_long == n_long), (name, g.csc.n_long)
        out.append((name, g))
    deg = degrees(out[2][1].csc).tolist()
    assert len(deg) <= 40 and all(k in deg for k in (0, 1, 15, 16, 17, 33, 255, 256, 257))
    d16 = out[3][1].csc
    assert sorted(degrees(d16)[d16.long_rows.cpu().long()].tolist()) == [17, 33, 255, 256, 257]     # a row is long ABOVE the chunk: 16 stays short
    return tuple(out)


def degrees(d):
    ip = d.indptr.cpu().long()
    return ip[1:] - ip[:-1]


def rows_of(d):
    return torch.repeat_interleave(torch.arange(d.n_rows), degrees(d))


def lane_steps(d):
    """L per row: how many edges one lane walks, ceil(deg / 16) for a short row, ceil(deg / 256) for a long one."""
    deg = degrees(d)
    return torch.where(deg > d.chunk, (deg + kBlock - 1) // kBlock, (deg + kRowLanes - 1) // kRowLanes).clamp(min=1)


def lane_stride(d):
    """The distance between two positions that share a lane, per row."""
    deg = degrees(d)
    return torch.where(deg > d.chunk, torch.full_like(deg, kBlock), torch.full_like(deg, kRowLanes))


def _perm(p, n):
    return torch.arange(n) if p is None else p.cpu().long()


def random_perm(n, seed):
    return torch.randperm(n, generator=torch.Generator().manual_seed(seed)).to(torch.int32)


# ------------------------------------------------------------------------------------------------ the contracts, float64
def z32_of(d, el, er, ee, eperm):
    """z in float32 in the kernel's own order, (er[row] + el[src]) + ee[eperm[k]]: IEEE additions, so bit for bit the kernel's z.  The
    sign of z is taken from it (zsign, the backward's gate): near z = 0 a float64 sum may have the other sign.  [nnz, H] or None."""
    rows, src, ep = rows_of(d), d.indices.cpu().long(), _perm(eperm, d.nnz)
    z = None
    for t, idx in ((er, rows), (el, src), (ee, ep)):
        if t is not None:
            v = t.detach().cpu().float()[idx]
            z = v if z is None else z + v
    return z


def forward64(d, el, er, ee, eperm, keep, slope, H, aperm):
    """The forward contract from float32 (or float64) operands, in float64: z = er[row] + el[src] + ee[eperm[k]], e = z if z > 0 else
    slope z, a = softmax of e over the kept positions of the row per head, written at aperm[k]; keep[eperm[k]] == 0: 0.  Non-finite
    logits follow the kernel's stated rules: a -inf logit is a dropped edge; a NaN or +inf logit makes every live entry of its (row,
    head) NaN; a (row, head) with nothing live gives zeros.  -> dict: a [nnz, H] (at aperm), zsign uint8 [nnz] (at aperm; H <= 8) or
    None, and in POSITION order: e, live, zabs = |er| + |el| + |ee|, M [n_rows, H] (0 where nothing is live)."""
    nnz, n = d.nnz, d.n_rows
    rows, src, ep, ap = rows_of(d), d.indices.cpu().long(), _perm(eperm, nnz), _perm(aperm, nnz)
    z, zabs = torch.zeros(nnz, H, dtype=F64), torch.zeros(nnz, H, dtype=F64)
    for t, idx in ((er, rows), (el, src), (ee, ep)):
        if t is not None:
            v = t.detach().cpu().double()[idx]
            z, zabs = z + v, zabs + v.abs()
    s64 = float(np.float32(slope))
    z32 = z32_of(d, el, er, ee, eperm)
    pos = z32 > 0
    e = torch.where(pos, z, z * s64)
    kept = torch.ones(nnz, dtype=torch.bool) if keep is None else keep.cpu()[ep] != 0
    live = kept.view(-1, 1) & ~torch.isneginf(e)
    bad_e = live & (torch.isnan(e) | torch.isposinf(e))
    idx = rows.view(-1, 1).expand(-1, H)
    fin = live & ~bad_e
    em = torch.where(fin, e, torch.full((), -np.inf, dtype=F64))
    M = torch.full((n, H), -np.inf, dtype=F64).scatter_reduce(0, idx, em, "amax", include_self=True)
    M = torch.where(torch.isneginf(M), torch.zeros((), dtype=F64), M)
    ex = torch.where(fin, torch.exp(torch.where(fin, e, torch.zeros((), dtype=F64)) - M[rows]), torch.zeros((), dtype=F64))
    den = torch.zeros(n, H, dtype=F64).index_add_(0, rows, ex)
    a = torch.where(fin, ex / den[rows].clamp(min=1e-300), torch.zeros((), dtype=F64))
    bad = torch.zeros(n, H, dtype=F64).index_add_(0, rows, bad_e.double()) > 0
    a = torch.where(bad[rows] & live, torch.full((), np.nan, dtype=F64), a)
    out = torch.zeros(nnz, H, dtype=F64)
    out[ap] = a
    zsign = None
    if H <= 8:
        bits = ((pos & kept.view(-1, 1)).long() << torch.arange(H)).sum(1).to(torch.uint8)
        zsign = torch.zeros(nnz, dtype=torch.uint8)
        zsign[ap] = bits
    return dict(a=out, a_pos=a, zsign=zsign, e=e, live=live, zabs=zabs, M=M, gate=pos)


def backward64(d, a, da, aperm, zperm, slope, H, gate=None, want_der=True):
    """The backward contract in float64 from the GIVEN float32 a and da ([nnz, H], indexed through aperm): t = sum a da per row and
    head, dz = a (da - t), times slope where not z > 0 (`gate`: bool [nnz, H] in position order, see z32_of; None with slope 1),
    written at zperm[k]; der = sum dz.  -> dict dz (at zperm), der, and in position order dz_pos, a_pos, sabs = sum |a da| per row."""
    nnz, n = d.nnz, d.n_rows
    rows, ap, zp = rows_of(d), _perm(aperm, nnz), _perm(zperm, nnz)
    a_, da_ = a.detach().cpu().double()[ap], da.detach().cpu().double()[ap]
    t = torch.zeros(n, H, dtype=F64).index_add_(0, rows, a_ * da_)
    sabs = torch.zeros(n, H, dtype=F64).index_add_(0, rows, (a_ * da_).abs())
    dz = a_ * (da_ - t[rows])
    s64 = float(np.float32(slope))
    if s64 != 1.0:
        assert gate is not None
        dz = torch.where(gate, dz, dz * s64)
    out = torch.zeros(nnz, H, dtype=F64)
    out[zp] = dz
    der = torch.zeros(n, H, dtype=F64).index_add_(0, rows, dz) if want_der else None
    return dict(dz=out, der=der, dz_pos=dz, a_pos=a_, da_pos=da_, sabs=sabs)


def segment_sum64(d, vals, perm=None):
    """out[r, :] = sum over the positions k of row r of vals[perm[k], :], float64."""
    v = vals.detach().cpu().double()[_perm(perm, d.nnz)]
    return torch.zeros(d.n_rows, vals.shape[1], dtype=F64).index_add_(0, rows_of(d), v)


def drop_seed(seed, seed_offset=None):
    """The Philox key: drop_seed, plus seed_offset * 0x9E3779B97F4A7C15 mod 2^64 when the device word is set."""
    return (int(seed) & M64) if seed_offset is None else ((int(seed) & M64) + int(seed_offset) * GOLDEN) & M64


def drop_mask(nnz, H, p, seed, seed_offset=None):
    """The attention-dropout keep mask, bool [nnz, H], indexed by the RECORD of `a` (aperm[k]): record r, head h is kept iff
    float32((w >> 8) * 2^-24) >= float32(p), w = word h % 4 of Philox4x32-10(key, counter r * ((H + 3) // 4) + h // 4)."""
    nq = (H + 3) // 4
    ctr = (np.arange(nnz, dtype=np.uint64)[:, None] * np.uint64(nq) + np.arange(nq, dtype=np.uint64)[None, :]).reshape(-1)
    w = philox4x32_10(drop_seed(seed, seed_offset), ctr).reshape(nnz, nq * 4)[:, :H]
    u = ((w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)
    return torch.from_numpy(u >= np.float32(p))


def drop_scale(p):
    """1 / (1 - p) as the kernel forms it, in float32."""
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


# ------------------------------------------------------------------------------------------------ bounds for seeded inputs
def forward_bounds(d, fwd, expf_err=None):
    """Per-entry bound on |kernel - forward64| for the weights, [nnz, H] in POSITION order, from the lengths and magnitudes of the
    restatement alone.  Derivation (first order, then expm1 of the total so that it also holds where it is not small):

    - The float32 logit.  z is two additions and e one product by the slope: |e32 - e| <= eta = U (2 zabs + |e|), zabs = |er| + |el| +
      |ee|.  Everything after it is a function of the STORED e32, so this enters once: moving every logit of a row by at most eta_row
      = max eta moves a weight by a relative 2 eta_row at most (numerator and denominator).
    - The exponentials.  The term of edge k in its lane's sum is a product of its own expf(e - m) and every later rescale expf(m -
      m'), then the lane combine expf(m - M): at most L + 1 calls, L the number of edges the lane walks; the numerator expf(e - M) is
      one more.  Each call is within EXPF_ERR (relative, 2 x measured).  Each ARGUMENT is one rounded subtraction, U |m - m'|; the
      running maximum only grows, so the arguments of a term's chain add up to exactly M - e_k and their roundings to at most U (M -
      e_k) <= U R, R the row's logit range; the same for the numerator.  Together (L + 2) EXPF_ERR + 2 U R.
    - The arithmetic.  A lane's step is one product and one sum (2 U, or U fused), L times; the combine's product, at most 9 additions
      across the lanes (4 shuffle steps of a group; 6 + 3 of a workgroup), the reciprocal and the final product: (2 L + 12) U.

        rel = (L + 2) EXPF_ERR + 2 U R + 2 eta_row + (2 L + 12) U,      bound = expm1(rel) a + TINY

    The issue's sketch multiplied eta by 2 (L + 1) as well; read against the kernel the logit's own error does not repeat along the
    chain (the chain telescopes in the stored logits), so it is counted once here - the tighter of the two readings.  Weights whose
    exponential is a subnormal number (below 2^-126 of the row's largest) have no relative accuracy in any float32 evaluation: TINY
    holds those absolutely."""
    expf_err = EXPF_ERR if expf_err is None else expf_err
    rows = rows_of(d)
    n, H = d.n_rows, fwd["e"].shape[1]
    idx = rows.view(-1, 1).expand(-1, H)
    live, e = fwd["live"], fwd["e"]
    eta = U * (2 * fwd["zabs"] + e.abs())
    zero = torch.zeros((), dtype=F64)
    eta_row = torch.zeros(n, H, dtype=F64).scatter_reduce(0, idx, torch.where(live, eta, zero), "amax", include_self=True)
    lo = torch.full((n, H), np.inf, dtype=F64).scatter_reduce(0, idx, torch.where(live, e, torch.full((), np.inf, dtype=F64)), "amin", include_self=True)
    R = torch.where(torch.isinf(lo), zero, fwd["M"] - lo)
    L = lane_steps(d).double().view(-1, 1)
    rel = (L + 2) * expf_err + 2 * U * R + 2 * eta_row + (2 * L + 12) * U
    return dict(rel=rel, a=torch.expm1(rel)[rows] * fwd["a_pos"] + TINY)


def backward_bounds(d, bwd, extra=0):
    """Per-entry bounds for dz ([nnz, H], position order) and der, pure arithmetic since a and da are given: t is a sum of deg fused
    products in some order, (deg + 3) U sum |a da|; dz = a (da - t) adds the subtraction, the product and the slope, 3 U |dz|:

        |dz - dz64| <= U [(deg + 3) a_k sum |a da| + 3 |dz64|]          (+ `extra` U a_k |da_k|: da was itself a rounded product)

    der adds (deg + 3) U sum |dz64| and the sum of its row's dz bounds.  Relative roundings say nothing of a product that underflows (a
    weight of 1e-44 is a given input at logit scale 1e3): each of the four operations behind a dz may lose up to the smallest normal
    number, 2^-126, if subnormal results are flushed, and so may each of the deg products of t - an absolute (deg + 4) 2^-126 per entry."""
    rows = rows_of(d)
    deg = degrees(d).double().view(-1, 1)
    dz = U * ((deg + 3)[rows] * bwd["a_pos"].abs() * bwd["sabs"][rows] + 3 * bwd["dz_pos"].abs() + extra * (bwd["a_pos"] * bwd["da_pos"]).abs())
    dz = dz + (deg + 4)[rows] * 2.0 ** -126                                  # and t's deg products likewise
    n, H = d.n_rows, dz.shape[1]
    tot = lambda x: torch.zeros(n, H, dtype=F64).index_add_(0, rows, x)
    return dict(dz=dz, der=(deg + 3) * U * tot(bwd["dz_pos"].abs()) + tot(dz))


def normal_inputs(g, H, seed, scale=1.0):
    """Seeded normal el [n_src, H], er [n_dst, H], ee [E, H] times `scale`, and unit-normal da [E, H]."""
    gen = torch.Generator().manual_seed(seed)
    r = lambda *shape: torch.randn(shape, generator=gen)
    E = g.number_of_edges()
    return r(g.number_of_src_nodes(), H) * scale, r(g.number_of_dst_nodes(), H) * scale, r(E, H) * scale, r(E, H)


def pick(names, el, er, ee):
    """The operands of a subset, the others None."""
    return tuple(t if n in names else None for n, t in (("el", el), ("er", er), ("ee", ee)))


# ------------------------------------------------------------------------------------------------ the exact regimes
def _ints(rng, lo, hi, shape):
    return torch.from_numpy(rng.integers(lo, hi + 1, shape).astype(np.float32))


def keep_mask(d, kind, seed):
    """uint8 [nnz] keep masks of the exact regimes: None, "random" (about a third dropped), "row" (random, and every position of the
    longest row and of row 0 dropped), "none" (every edge dropped).  Indexed by eperm[k]; the caller permutes."""
    if kind is None:
        return None
    rng = np.random.default_rng(seed)
    k = (rng.random(d.nnz) >= 0.35).astype(np.uint8)
    if kind == "row":
        deg, ip = degrees(d), d.indptr.cpu().long()
        for r in {int(deg.argmax()), 0}:
            k[int(ip[r]):int(ip[r + 1])] = 0
    if kind == "none":
        k[:] = 0
    return torch.from_numpy(k)


def equal_logit_inputs(d, n_src, H, names, eperm, keep, seed, slope=0.25):
    """Exact regime 1: integer-valued el, er, ee such that z is CONSTANT over the positions of every (row, head) - the constants are
    drawn from -2 .. 2, so z == 0 occurs - whichever subset `names` of the three is given.  Every kept weight is then float32(1) /
    float32(kept count) entry for entry: expf(0) is 1, the count is an exact sum of ones, and the division is correctly rounded.
    `keep`: uint8 [nnz] indexed like ee (by eperm[k]) or None.  -> (el, er, ee, want [nnz, H] float32 in POSITION order, z [nnz, H])."""
    rng = np.random.default_rng(seed)
    nnz, n = d.nnz, d.n_rows
    rows, src, ep = rows_of(d), d.indices.cpu().long(), _perm(eperm, nnz)
    c = _ints(rng, -2, 2, (n, H))
    er = _ints(rng, -8, 8, (n, H)) if "er" in names else None
    el = ee = None
    if "ee" in names:
        el = _ints(rng, -8, 8, (n_src, H)) if "el" in names else None
        rest = c[rows] - (0 if el is None else el[src]) - (0 if er is None else er[rows])
        ee = torch.zeros(nnz, H)
        ee[ep] = rest
    elif "el" in names:
        el = _ints(rng, -2, 2, (1, H)).expand(n_src, H).contiguous()        # no per-edge term: every source carries the same value
    z = z32_of(d, el, er, ee, eperm)
    zr = torch.zeros(n, H).index_add_(0, rows, z)
    deg = degrees(d).float().view(-1, 1)
    assert bool((z * deg[rows] == zr[rows]).all()), "z is not constant over a row"
    assert float(z.abs().max()) <= 20 if nnz else True
    kept = torch.ones(nnz) if keep is None else (keep[ep] != 0).float()
    count = torch.zeros(n).index_add_(0, rows, kept)
    want = (kept / count.clamp(min=1)[rows]).view(-1, 1).expand(-1, H).contiguous()       # float32 division of two exact integers
    return el, er, ee, want, z


def spike_positions(d, mode):
    """The positions of the spikes of every non-empty row.  first / last: the row's first / last position; second: the position one
    lane stride after the first (the second edge of lane 0; the last position where the row is shorter); alone: the middle of the row
    (in a row of 17 .. 31 its lane holds no other edge); ties: all four."""
    ip, deg, stride = d.indptr.cpu().long(), degrees(d), lane_stride(d)
    out = []
    for r in range(d.n_rows):
        b, n = int(ip[r]), int(deg[r])
        if n == 0:
            continue
        cand = dict(first=[0], last=[n - 1], second=[min(int(stride[r]), n - 1)], alone=[n // 2])
        cand["ties"] = sorted({p for v in cand.values() for p in v})
        out.extend(b + p for p in cand[mode])
    return torch.tensor(out, dtype=torch.int64)


def spike_inputs(d, H, mode, eperm, seed, with_er=True):
    """Exact regime 2: ee integer-valued in -8 .. 8 except at the spikes of every row (`spike_positions`), which are 300: at least 200
    above the rest after the leaky ReLU (slope 0.25) and after the row's er (an integer in -8 .. 8, the same for the whole row).
    expf of -200 or less is 0 in float32, so each of the t spikes of a row gets float32(1) / float32(t) and every other entry exactly
    0.  -> (er, ee, want [nnz, H] float32 in position order)."""
    rng = np.random.default_rng(seed)
    nnz, n = d.nnz, d.n_rows
    rows, ep = rows_of(d), _perm(eperm, nnz)
    er = _ints(rng, -8, 8, (n, H)) if with_er else None
    base = _ints(rng, -8, 8, (nnz, H))
    sp = spike_positions(d, mode)
    hot = torch.zeros(nnz)
    hot[sp] = 1
    base[sp] = 300.0
    ee = torch.zeros(nnz, H)
    ee[ep] = base
    z = z32_of(d, None, er, ee, eperm)
    e = torch.where(z > 0, z, z * 0.25)
    top = torch.full((n, H), -np.inf).scatter_reduce(0, rows.view(-1, 1).expand(-1, H), e, "amax", include_self=True)
    assert bool(((e == top[rows]) == (hot.view(-1, 1) > 0)).all()) and bool((top[rows] - e)[hot == 0].min() >= 200 if (hot == 0).any() else True)
    count = torch.zeros(n).index_add_(0, rows, hot)
    want = (hot / count.clamp(min=1)[rows]).view(-1, 1).expand(-1, H).contiguous()
    return er, ee, want


def integer_backward_inputs(d, n_src, H, seed):
    """Exact regime 3: a in 0 .. 3, da in -4 .. 4, el / er / ee integers in -2 .. 2 (sums that are exactly 0 occur; asserted), for a
    slope of 0.25, 1 or 0.  Every product and sum is then exact: ASSERTED, the absolute terms of every compared sum stay below 2^22 (they
    are multiples of 0.25) and t below 2^24.  -> (el, er, ee, a, da), a and da in the order of the records (the caller's aperm)."""
    rng = np.random.default_rng(seed)
    nnz, n = d.nnz, d.n_rows
    el, er, ee = _ints(rng, -2, 2, (n_src, H)), _ints(rng, -2, 2, (n, H)), _ints(rng, -2, 2, (nnz, H))
    a, da = _ints(rng, 0, 3, (nnz, H)), _ints(rng, -4, 4, (nnz, H))
    return el, er, ee, a, da


def assert_backward_exact(d, bwd):
    """The conditions of regime 3 for one restated backward."""
    rows = rows_of(d)
    n, H = d.n_rows, bwd["dz_pos"].shape[1]
    if d.nnz == 0:
        return
    assert float(bwd["sabs"].max()) < 2.0 ** 24
    assert float(bwd["dz_pos"].abs().max()) < EXACT_LIMIT
    assert float(torch.zeros(n, H, dtype=F64).index_add_(0, rows, bwd["dz_pos"].abs()).max()) < EXACT_LIMIT


def integer_vals(nnz, W, seed):
    """Exact regime 4: integer-valued records in -8 .. 8; a row of at most 2^18 of them sums exactly in any order."""
    return _ints(np.random.default_rng(seed), -8, 8, (nnz, W))


# ------------------------------------------------------------------------------------------------ non-finite logits
def lane_positions(d, row):
    """For one row: (first on a shared lane, second on that lane, alone on its lane) as positions, or None where the row has none."""
    b, deg, stride = int(d.indptr[row]), int(degrees(d)[row]), int(lane_stride(d)[row])
    shared = b if deg > stride else None
    second = b + stride if deg > stride else None
    p = min(deg, stride) - 1                                            # the last lane in use: alone unless the row wraps onto it
    alone = b + p if (deg > 0 and p + stride >= deg) else None
    return shared, second, alone
