"""The GAT attention and segment-sum kernels (csrc/attn.hip) on the MI355X against the float64 restatements of tests/attn_cases.py:
entry for entry in the exact regimes (equal logits, spikes, integer backward, integer segment sum) at every head-tile count, logit
subset, permutation and row class; the zsign byte and the backward that reads it against the backward that recomputes z; offset
(4- and 8-byte) views against aligned ones, bit for bit; seeded normal inputs under the derived bounds; the attention-dropout mask
against its numpy Philox restatement; and the rules for non-finite logits.  Called through `_C.gat_attn_fwd`, `_C.gat_attn_bwd` and
`_C.segment_sum` directly.

Largest error seen as a fraction of its derived bound (run with -s to print them; DESIGN §8 "Attention and segment sum"): weights 0.145
at logit scale 1 and 0.298 at 1e3, dz 0.390 / 0.370, der 0.272 / 0.182, with attention dropout dz 0.341 and der 0.242, segment sum 0.273.
The device library's expf on [-87, 0]: 1.1219e-07 = 1.88 U (tests/attn_cases.EXPF_MEASURED)."""
import functools

import numpy as np
import pytest
import torch

from bot_amd import _C, ops
from tests import attn_cases as AC

pytestmark = pytest.mark.gpu
DEV = "cuda"
U = AC.U
WORST = {}
SLOPES = (0.25, 1.0, 0.0)


@functools.lru_cache(maxsize=None)
def _graphs():
    """(name, CPU graph, device graph) of tests/attn_cases.graphs(), both directions built once on the CPU."""
    out = []
    for name, g in AC.graphs():
        g.create_formats_()
        out.append((name, g, g.to(DEV)))
    return tuple(out)


def _d(t):
    return None if t is None else t.to(DEV)


def _same(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _pos(t, perm):
    """Records -> position order."""
    return t if perm is None else t[perm.long().to(t.device)]


def _worst(name, err, bound):
    if err.numel():
        WORST[name] = max(WORST.get(name, 0.0), float((err / bound.clamp(min=1e-300)).max()))


def _perms(nnz, i, seed):
    """(eperm, aperm, zperm): each None or a random permutation, every combination over i = 0 .. 7."""
    return tuple(AC.random_perm(nnz, seed + j) if (i >> j) & 1 else None for j in range(3))


# ------------------------------------------------------------------------------------------------ 1. exact regimes
@pytest.mark.parametrize("H", AC.HEADS)
def test_equal_logits_are_exact_fp64(H):
    """Regime 1: every kept weight is float32(1) / float32(kept count) and every dropped one 0, bit for bit, for all seven logit
    subsets, keep masks that drop a third, whole rows and everything, and the zsign byte (z == 0 occurs) equals the restatement's."""
    for gi, (name, g, gd) in enumerate(_graphs()):
        d, dd, nnz, n_src = g.csc, gd.csc, g.number_of_edges(), g.number_of_src_nodes()
        for si, names in enumerate(AC.SUBSETS):
            seed = 100 * gi + 10 * si + H
            eperm, aperm, _ = _perms(nnz, gi + si, seed)
            keep = AC.keep_mask(d, (None, "random", "row", "none")[(gi + si) % 4], seed)
            el, er, ee, want, z = AC.equal_logit_inputs(d, n_src, H, names, eperm, keep, seed)
            zs = torch.full((nnz,), 255, dtype=torch.uint8, device=DEV) if H <= 8 else None
            a = _C.gat_attn_fwd(dd, _d(el), _d(er), _d(ee), _d(eperm), _d(keep), 0.25, H, _d(aperm), zs)
            assert torch.equal(_pos(a, aperm).cpu(), want), (name, names, H)
            if zs is not None:
                assert torch.equal(zs.cpu(), AC.forward64(d, el, er, ee, eperm, keep, 0.25, H, aperm)["zsign"]), (name, names, H)


@pytest.mark.parametrize("H", AC.HEADS)
def test_spikes_are_exact_fp64(H):
    """Regime 2: the t spikes of a row get 1 / t and every other entry exactly 0, with the spike first, second and last on its lane,
    alone on a lane, and tied across lanes (the running maximum jumps at a chosen step of the lane's walk)."""
    for gi, (name, g, gd) in enumerate(_graphs()):
        d, dd, nnz = g.csc, gd.csc, g.number_of_edges()
        for mi, mode in enumerate(("first", "second", "alone", "last", "ties")):
            eperm, aperm, _ = _perms(nnz, gi + mi, gi)
            er, ee, want = AC.spike_inputs(d, H, mode, eperm, 7 * gi + mi + H, with_er=mi % 2 == 0)
            a = _C.gat_attn_fwd(dd, None, _d(er), _d(ee), _d(eperm), None, 0.25, H, _d(aperm))
            assert torch.equal(_pos(a, aperm).cpu(), want), (name, mode, H)


@pytest.mark.parametrize("H", AC.HEADS)
def test_integer_backward_is_exact_fp64(H):
    """Regime 3: dz and der entry for entry, for all seven sources of the recomputed sign, three slopes, der on and off."""
    for gi, (name, g, gd) in enumerate(_graphs()):
        d, dd, nnz, n_src = g.csc, gd.csc, g.number_of_edges(), g.number_of_src_nodes()
        el, er, ee, a, da = AC.integer_backward_inputs(d, n_src, H, 3 * gi + H)
        ad, dad = _d(a), _d(da)
        for si, names in enumerate(AC.SUBSETS):
            eperm, aperm, zperm = _perms(nnz, gi + si, gi + si)
            pel, per, pee = AC.pick(names, el, er, ee)
            gate = AC.z32_of(d, pel, per, pee, eperm) > 0
            for li, slope in enumerate(SLOPES):
                want_der = (gi + si + li) % 3 != 0
                bwd = AC.backward64(d, a, da, aperm, zperm, slope, H, gate=gate, want_der=want_der)
                AC.assert_backward_exact(d, bwd)
                dz, der = _C.gat_attn_bwd(dd, _d(pel), _d(per), _d(pee), _d(eperm), slope, H, ad, dad, _d(aperm), _d(zperm), want_der)
                assert torch.equal(dz.cpu().double(), bwd["dz"]), (name, names, slope, H)
                assert (der is None) == (not want_der) and (der is None or torch.equal(der.cpu().double(), bwd["der"])), (name, names, slope, H)


@pytest.mark.parametrize("W", AC.HEADS)
def test_integer_segment_sum_is_exact_fp64(W):
    """Regime 4, over the CSC and the CSR, with perm None, the direction's edge ids and csr2csc."""
    for gi, (name, g, gd) in enumerate(_graphs()):
        nnz = g.number_of_edges()
        vals = AC.integer_vals(nnz, W, gi + W)
        for dn, pn in (("csc", None), ("csc", "eid"), ("csr", None), ("csr", "eid"), ("csr", "csr2csc"), ("csc", "csr2csc")):
            d, dd = getattr(g, dn), getattr(gd, dn)
            perm = None if pn is None else (g.csr2csc if pn == "csr2csc" else d.eid)
            out = _C.segment_sum(dd, _d(vals), _d(perm))
            assert torch.equal(out.cpu().double(), AC.segment_sum64(d, vals, perm)), (name, dn, pn, W)


# ------------------------------------------------------------------------------------------------ 2. zsign
@pytest.mark.parametrize("H", [h for h in AC.HEADS if h <= 8])
def test_zsign_bytes_and_the_backward_that_reads_them_fp64(H):
    """The bytes the forward writes equal the restatement's (bit j = [z_j > 0], 0 for a dropped edge), on integer logits (z == 0
    occurs) and on seeded ones; the backward that reads them is bit-identical to the backward that recomputes z."""
    hit_zero = False
    for gi, (name, g, gd) in enumerate(_graphs()):
        d, dd, nnz, n_src = g.csc, gd.csc, g.number_of_edges(), g.number_of_src_nodes()
        for kind in ("int", "normal"):
            if kind == "int":
                el, er, ee, _, da = AC.integer_backward_inputs(d, n_src, H, gi + H)
            else:
                el, er, ee, da = AC.normal_inputs(g, H, gi + H)
            eperm, aperm, zperm = _perms(nnz, gi + 1, gi)
            keep = AC.keep_mask(d, (None, "random", "row")[gi % 3], gi)
            z = AC.z32_of(d, el, er, ee, eperm)
            hit_zero |= bool((z == 0).any())
            zs = torch.full((nnz,), 255, dtype=torch.uint8, device=DEV)
            a = _C.gat_attn_fwd(dd, _d(el), _d(er), _d(ee), _d(eperm), _d(keep), 0.25, H, _d(aperm), zs)
            assert torch.equal(zs.cpu(), AC.forward64(d, el, er, ee, eperm, keep, 0.25, H, aperm)["zsign"]), (name, kind, H)
            for slope in (0.25, 0.0):
                dz1, der1 = _C.gat_attn_bwd(dd, _d(el), _d(er), _d(ee), _d(eperm), slope, H, a, _d(da), _d(aperm), _d(zperm), True, zsign=zs)
                dz2, der2 = _C.gat_attn_bwd(dd, _d(el), _d(er), _d(ee), _d(eperm), slope, H, a, _d(da), _d(aperm), _d(zperm), True)
                dz3, _ = _C.gat_attn_bwd(dd, None, None, None, None, slope, H, a, _d(da), _d(aperm), _d(zperm), False, zsign=zs)
                assert _same(dz1, dz2) and _same(der1, der2) and _same(dz3, dz1), (name, kind, slope, H)
    assert hit_zero


# ------------------------------------------------------------------------------------------------ 3. alignment
def _offset(t, k):
    """A contiguous device view of `t` that starts 4 k bytes past a 16-byte boundary."""
    buf = torch.empty(t.numel() + 8, dtype=t.dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[k:k + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == (4 * k) % 16
    return v


@pytest.mark.parametrize("H", [2, 4, 6, 8])
def test_offset_views_equal_aligned_ones_fp64(H):
    """Even H <= 8 moves records as 8- or 16-byte vectors only when every base is 16-byte aligned; an offset view of el, ee, a or da
    takes the scalar path and must give the same bits; likewise segment_sum's vals."""
    for gi, (name, g, gd) in enumerate(_graphs()[:6]):
        dd, nnz = gd.csc, g.number_of_edges()
        el, er, ee, da = (_d(t) for t in AC.normal_inputs(g, H, gi))
        eperm, aperm, zperm = (_d(p) for p in _perms(nnz, 7, gi))
        a0 = _C.gat_attn_fwd(dd, el, er, ee, eperm, None, 0.2, H, aperm)
        dz0, der0 = _C.gat_attn_bwd(dd, el, er, ee, eperm, 0.2, H, a0, da, aperm, zperm, True)
        s0 = _C.segment_sum(gd.csr, dz0, gd.csr2csc)
        for k in (1, 2):
            for which in ("el", "ee", "both"):
                a = _C.gat_attn_fwd(dd, _offset(el, k) if which != "ee" else el, er, _offset(ee, k) if which != "el" else ee, eperm, None, 0.2, H, aperm)
                assert _same(a, a0), (name, H, k, which)
            for which in ("a", "da", "el"):
                dz, der = _C.gat_attn_bwd(dd, _offset(el, k) if which == "el" else el, er, ee, eperm, 0.2, H, _offset(a0, k) if which == "a" else a0,
                                          _offset(da, k) if which == "da" else da, aperm, zperm, True)
                assert _same(dz, dz0) and _same(der, der0), (name, H, k, which)
            assert _same(_C.segment_sum(gd.csr, _offset(dz0, k), gd.csr2csc), s0), (name, H, k)


# ------------------------------------------------------------------------------------------------ 4. seeded inputs under the bounds
def _seeded(name, g, gd, H, seed, scale, names, tag):
    d, dd, nnz = g.csc, gd.csc, g.number_of_edges()
    el, er, ee, da = AC.normal_inputs(g, H, seed, scale)
    el, er, ee = AC.pick(names, el, er, ee)
    eperm, aperm, zperm = _perms(nnz, seed, seed)
    keep = AC.keep_mask(d, (None, "random")[seed % 2], seed)
    a = _C.gat_attn_fwd(dd, _d(el), _d(er), _d(ee), _d(eperm), _d(keep), 0.2, H, _d(aperm))
    fwd = AC.forward64(d, el, er, ee, eperm, keep, 0.2, H, aperm)
    fb = AC.forward_bounds(d, fwd)
    err = (_pos(a, aperm).cpu().double() - fwd["a_pos"]).abs()
    _worst(f"a {tag}", err, fb["a"])
    assert bool((err <= fb["a"]).all()), (name, H, names, float((err / fb["a"]).max()))
    dz, der = _C.gat_attn_bwd(dd, _d(el), _d(er), _d(ee), _d(eperm), 0.2, H, a, _d(da), _d(aperm), _d(zperm), True)
    bwd = AC.backward64(d, a.cpu(), da, aperm, zperm, 0.2, H, gate=fwd["gate"])
    bb = AC.backward_bounds(d, bwd)
    e_dz, e_der = (_pos(dz, zperm).cpu().double() - bwd["dz_pos"]).abs(), (der.cpu().double() - bwd["der"]).abs()
    _worst(f"dz {tag}", e_dz, bb["dz"]), _worst(f"der {tag}", e_der, bb["der"])
    assert bool((e_dz <= bb["dz"]).all()) and bool((e_der <= bb["der"]).all()), (name, H, names)
    vals = torch.randn(nnz, H, generator=torch.Generator().manual_seed(seed))
    out = _C.segment_sum(gd.csr, _d(vals), gd.csr2csc)
    s64 = AC.segment_sum64(g.csr, vals, g.csr2csc)
    sb = (AC.degrees(g.csr).double().view(-1, 1) + 3) * U * AC.segment_sum64(g.csr, vals.abs(), g.csr2csc)
    e_s = (out.cpu().double() - s64).abs()
    _worst(f"segment_sum {tag}", e_s, sb)
    assert bool((e_s <= sb).all()), (name, H)
    return a


@pytest.mark.parametrize("scale", [1.0, 1e3])
@pytest.mark.parametrize("H", [1, 3, 4, 6, 8, 9, 17])
def test_seeded_inputs_against_fp64_under_derived_bounds(H, scale):
    for gi, (name, g, gd) in enumerate(_graphs()):
        _seeded(name, g, gd, H, gi + H, scale, AC.SUBSETS[(gi + H) % 7], f"scale {scale:g}")
    print("largest error / bound so far:", {k: round(v, 4) for k, v in sorted(WORST.items())})


def test_expf_error_measured_fp64():
    """The device library's expf against float64 exp: two-edge rows with logits (0, t), t a seeded float32 grid on [-87, 0] (and the
    end points); the ratio of the two weights is expf(t) up to the rounding of one product (the weight of logit 0 is 1 / sum exactly).
    The largest relative error must stay within tests/attn_cases.EXPF_MEASURED, which the bounds double; on [-104, -87] the result is
    a subnormal number and is held absolutely, to 2^-126 of the row's sum."""
    import bot_amd
    n = 1500
    gen = torch.Generator().manual_seed(0)
    t = -87.0 * torch.rand(n, generator=gen)
    t[:4] = torch.tensor([-87.0, -1.0, -2.0 ** -20, -0.5])
    src = torch.zeros(2 * n, dtype=torch.int64)
    dst = torch.arange(n).repeat_interleave(2)
    g = bot_amd.Graph(src, dst, n).to(DEV)
    assert g.csc.n_long == 0 and bool((g.csc.eid.cpu() == torch.arange(2 * n)).all())
    for lo, hi in ((-87.0, 0.0), (-104.0, -87.0)):
        tt = t if lo == -87.0 else (lo + (hi - lo) * torch.rand(n, generator=gen))
        ee = torch.stack([torch.zeros(n), tt], 1).reshape(-1, 1)
        a = _C.gat_attn_fwd(g.csc, None, None, ee.to(DEV), None, None, 1.0, 1, None).cpu().double().view(n, 2)
        want = torch.exp(tt.double())
        if lo == -87.0:
            rel = ((a[:, 1] / a[:, 0] - want) / want).abs()
            print(f"expf on [-87, 0]: largest relative error of the weight ratio {float(rel.max()):.4e} = {float(rel.max()) / U:.3f} U at t = {float(tt[rel.argmax()])!r}")
            assert float(rel.max()) <= AC.EXPF_MEASURED
            assert float(rel.max()) <= 4 * U
        else:
            err = (a[:, 1] - want * a[:, 0]).abs()
            print(f"expf on [-104, -87]: largest absolute error {float(err.max()):.4e} = {float(err.max()) / 2.0 ** -149:.2f} x 2^-149")
            assert float(err.max()) <= 2.0 ** -126


# ------------------------------------------------------------------------------------------------ 5. attention dropout
@pytest.mark.parametrize("H", [1, 4, 6, 8, 9, 12])
def test_attention_dropout_against_the_philox_restatement_fp64(H):
    """a_drop == a * mask / (1 - p) with the mask from the numpy Philox restatement (counter record * ceil(H / 4) + h // 4, word h % 4),
    to rtol 1e-6 on kept entries and exactly 0 elsewhere; the backward with `drop` equals the float64 backward fed da * mask / (1 - p),
    under the backward bound.  Seeds above 2^32; the device word `_C.SEED_OFFSET` set and unset."""
    saved = _C.SEED_OFFSET
    try:
        for gi, (name, g, gd) in enumerate(_graphs()[2:4]):
            d, dd, nnz = g.csc, gd.csc, g.number_of_edges()
            el, er, ee, da = AC.normal_inputs(g, H, gi + H)
            for pi, p in enumerate((0.3, 0.5)):
                for off in (None, 5):
                    _C.SEED_OFFSET = None if off is None else torch.full((1,), off, dtype=torch.int64, device=DEV)
                    seed = 2 ** 40 + 12345 * H + pi
                    eperm, aperm, zperm = _perms(nnz, gi + pi + (off or 0), gi)
                    a, a_drop = _C.gat_attn_fwd(dd, _d(el), _d(er), _d(ee), _d(eperm), None, 0.2, H, _d(aperm), drop=(p, seed))
                    a_ref = _C.gat_attn_fwd(dd, _d(el), _d(er), _d(ee), _d(eperm), None, 0.2, H, _d(aperm))
                    assert _same(a, a_ref)
                    mask = AC.drop_mask(nnz, H, p, seed, off)
                    c = AC.drop_scale(p)
                    got, a_c = a_drop.cpu(), a.cpu()
                    assert bool((got[~mask] == 0).all()), (name, H, p, off)
                    np.testing.assert_allclose(got[mask].numpy(), (a_c.double() * c)[mask].numpy(), rtol=1e-6, atol=0)
                    rate = float(mask.double().mean())
                    assert abs(rate - (1 - p)) <= 5 * (p * (1 - p) / mask.numel()) ** 0.5
                    dz, der = _C.gat_attn_bwd(dd, _d(el), _d(er), _d(ee), _d(eperm), 0.2, H, a, _d(da), _d(aperm), _d(zperm), True, drop=(p, seed))
                    gate = AC.z32_of(d, el, er, ee, eperm) > 0
                    bwd = AC.backward64(d, a_c, da.double() * mask.double() * c, aperm, zperm, 0.2, H, gate=gate)
                    bb = AC.backward_bounds(d, bwd, extra=1)
                    e_dz, e_der = (_pos(dz, zperm).cpu().double() - bwd["dz_pos"]).abs(), (der.cpu().double() - bwd["der"]).abs()
                    _worst("dz dropout", e_dz, bb["dz"]), _worst("der dropout", e_der, bb["der"])
                    assert bool((e_dz <= bb["dz"]).all()) and bool((e_der <= bb["der"]).all()), (name, H, p, off)
    finally:
        _C.SEED_OFFSET = saved
    print("largest error / bound so far:", {k: round(v, 4) for k, v in sorted(WORST.items())})


# ------------------------------------------------------------------------------------------------ 6. non-finite logits
def _nonfinite_cases(d):
    """{kind: [(row, position)]} over every row with at least two in-edges: first / second on a shared lane, alone on its lane."""
    out = dict(first=[], second=[], alone=[])
    for r in range(d.n_rows):
        if int(AC.degrees(d)[r]) < 2:
            continue
        for kind, p in zip(("first", "second", "alone"), AC.lane_positions(d, r)):
            if p is not None:
                out[kind].append((r, p))
    return out


def _softmax_calls(g, gd, ee_pos, H):
    """The same position-ordered logits through `_C.gat_attn_fwd` and through `ops.edge_softmax` (edge-id order) -> position order."""
    d = gd.csc
    a1 = _C.gat_attn_fwd(d, None, None, ee_pos, None, None, 1.0, H, None)
    logits = torch.empty_like(ee_pos)
    logits[d.eid.long()] = ee_pos
    a2 = ops.edge_softmax(gd, logits.view(-1, H, 1)).view(-1, H)[d.eid.long()]
    return a1, a2


@pytest.mark.parametrize("gi", [2, 3])
@pytest.mark.parametrize("kind", ["first", "second", "alone"])
def test_nonfinite_logits_follow_the_stated_rules_fp64(gi, kind):
    """In both row classes (the lanes graph with chunk 300: short rows; with chunk 16: long rows), for a bad logit first and second on
    a shared lane and alone on its lane, in head 0 of H = 3:
    - a -inf logit among finite ones gets weight 0, the rest of the row is the softmax without it (forward bound), and its dz is 0;
    - a NaN or +inf logit makes every entry of its (row, head) NaN; other rows and other heads keep their bits;
    - a (row, head) whose logits are all -inf gives zeros."""
    name, g, gd = _graphs()[gi]
    d, dd, nnz, H = g.csc, gd.csc, g.number_of_edges(), 3
    _, _, ee, da = AC.normal_inputs(g, H, 9)
    rows = AC.rows_of(d)
    cases = _nonfinite_cases(d)[kind]
    long_rows = set(d.long_rows.tolist()) if d.n_long else set()
    assert cases and (gi == 2 or any(r in long_rows for r, _ in cases)) and (gi == 3 or any(r not in long_rows for r, _ in cases))
    hit = torch.zeros(nnz, H, dtype=torch.bool)
    for r, _ in cases:
        hit[rows == r, 0] = True
    clean = _C.gat_attn_fwd(dd, None, None, _d(ee), None, None, 1.0, H, None).cpu()
    for bad in (-np.inf, np.nan, np.inf):
        e2 = ee.clone()
        for _, p in cases:
            e2[p, 0] = bad
        for a in _softmax_calls(g, gd, _d(e2), H):
            got = a.cpu()
            assert _same(got[~hit], clean[~hit]), (name, kind, bad)
            if bad == -np.inf:
                fwd = AC.forward64(d, None, None, e2, None, None, 1.0, H, None)
                fb = AC.forward_bounds(d, fwd)
                for r, p in cases:
                    assert float(got[p, 0]) == 0, (name, kind, r, float(got[p, 0]), got[rows == r, 0][:20].tolist())
                assert bool(((got.double() - fwd["a"]).abs() <= fb["a"]).all()), (name, kind, "the row without the -inf edge")
                dz, der = _C.gat_attn_bwd(dd, None, None, _d(e2), None, 1.0, H, a, _d(da), None, None, True)
                assert all(float(dz[p, 0]) == 0 for _, p in cases) and bool(torch.isfinite(dz).all()) and bool(torch.isfinite(der).all())
            else:
                for r, p in cases:
                    assert bool(torch.isnan(got[rows == r, 0]).all()), (name, kind, bad, r, got[rows == r, 0][:20].tolist())
    e2 = ee.clone()
    e2[hit] = -np.inf
    for a in _softmax_calls(g, gd, _d(e2), H):
        got = a.cpu()
        assert bool((got[hit] == 0).all()) and _same(got[~hit], clean[~hit]), (name, kind, "all -inf")


@pytest.mark.parametrize("gi", [2, 3])
def test_gat_infer_on_nonfinite_logits_fp64(gi):
    """`_C.gat_infer` (csrc/infer.hip, its own softmax) on the same inputs: it agrees with the first two rules - a -inf logit among
    finite ones contributes nothing and the rest of the row is the softmax without it; a NaN or +inf logit makes its (row, head) NaN
    and touches nothing else - and DEPARTS from the third: a (row, head) whose logits are all -inf gives NaN, the reference's answer,
    where `gat_attn_fwd` gives zeros (DESIGN §8 "Attention and segment sum"; infer.hip is recorded here, not changed)."""
    name, g, gd = _graphs()[gi]
    d, dd, H, D = g.csc, gd.csc, 3, 4
    n_src = g.number_of_src_nodes()
    _, _, ee, _ = AC.normal_inputs(g, H, 9)
    x = torch.randn(n_src, H, D, generator=torch.Generator().manual_seed(1))
    el = torch.zeros(n_src, H, device=DEV)
    rows, src = AC.rows_of(d), d.indices.long()
    for kind, cases in _nonfinite_cases(d).items():
        if not cases:
            continue
        hit = torch.zeros(d.n_rows, H, dtype=torch.bool)
        for r, _ in cases:
            hit[r, 0] = True
        for bad in (-np.inf, np.nan, np.inf, "all"):
            e2 = ee.clone()
            for r, p in cases:
                if bad == "all":
                    e2[rows == r, 0] = -np.inf
                else:
                    e2[p, 0] = bad
            out = _C.gat_infer(dd, _d(x), el, None, _d(e2), slope=1.0).cpu().double()
            a = AC.forward64(d, None, None, e2, None, None, 1.0, H, None)["a"]
            want = torch.zeros(d.n_rows, H, D, dtype=torch.float64).index_add_(0, rows, a.unsqueeze(-1) * x.double()[src])
            tol = 1e-5 * torch.zeros(d.n_rows, H, D, dtype=torch.float64).index_add_(0, rows, torch.nan_to_num(a).unsqueeze(-1) * x.double()[src].abs()) + 1e-30
            assert bool(((out - want).abs()[~hit] <= tol[~hit]).all()), (name, kind, bad)
            if bad == -np.inf:
                assert bool(((out - want).abs()[hit] <= tol[hit]).all()), (name, kind, bad)
            else:
                assert bool(torch.isnan(out[hit]).all()), (name, kind, bad)     # "all": the reference's NaN, not gat_attn_fwd's zeros


# ------------------------------------------------------------------------------------------------ 7. sizes
def test_graph_without_edges_gives_zeros_fp64():
    """nnz == 0 with n_rows > 0: the backward's der and segment_sum are zeros (their outputs are written, not left as allocated)."""
    import bot_amd
    for n in (1, 15, 16, 17):
        g = bot_amd.Graph(torch.zeros(0, dtype=torch.int64), torch.zeros(0, dtype=torch.int64), n).to(DEV)
        for H in (1, 3, 9):
            e = torch.zeros(0, H, device=DEV)
            el = torch.randn(n, H, device=DEV)
            assert _C.gat_attn_fwd(g.csc, el, el, None, None, None, 0.2, H, None).shape == (0, H)
            dz, der = _C.gat_attn_bwd(g.csc, el, el, None, None, 0.2, H, e, e, None, None, True)
            assert dz.shape == (0, H) and der.shape == (n, H) and bool((der == 0).all())
            out = _C.segment_sum(g.csc, e, None)
            assert out.shape == (n, H) and bool((out == 0).all())
