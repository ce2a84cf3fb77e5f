"""The deferred form of the BatchNorm-backward by-product (include/bot_gnn.h "d h recomputed in the apply", bot_amd.gemm.DeferredDh) on the
MI355X: `d h = d out . W^T` of a short reduction is launched without its store (reduce-only: the partials of the storing launch, bit for
bit), and the epilogue's apply pass runs inside a second launch of the same product (apply mode: the bits `bn_act_bwd_apply_halves` writes
from the stored `d h`).

Kernel level: shapes with a ragged last row tile (257, 549, 4099, 1000 rows of 256-row tiles), a ragged last column tile (192 is whole, 750
and 300 are not), x rows of 8-byte (pitch 750) and 16-byte (752, 192, 300) alignment, row-major and fragment-major weights, one and two
scales, head blocks with and without padding columns, with and without the fp32 dx, batch and running statistics (NULL sums).
Layer level: the 3-layer arxiv-style stack on ~600 nodes, one train step with the switch on and off, everything bit for bit.

max|dx| is compared as the maximum over the by-product slots: WHICH slot a wave publishes into is a function of the launch's grid (common.h
absmax_publish), the value every consumer reads (halves_scale_from_slots) is the maximum over the set."""
import pytest
import torch
import torch.nn.functional as F

import bot_amd
from bot_amd import _C, gemm
from bot_amd import nn as bnn
from bot_amd.nn import fused
from bot_amd.synth import powerlaw_edges
from bot_amd.workloads import ARXIV_GAT

pytestmark = pytest.mark.gpu
DEV = "cuda"
SEED = 123456789
SENTINEL = 7.0
CASES = ((257, 64, 192, 192, 0.0, False, True), (549, 128, 750, 752, 0.75, True, True),
         (4099, 128, 750, 750, 0.5, True, False), (1000, 128, 300, 300, 0.0, True, True))


@pytest.mark.parametrize("m,K,F_,ldx,p,relu,affine", CASES)
def test_reduce_only_and_apply_mode_are_the_stored_form_bit_for_bit(m, K, F_, ldx, p, relu, affine):
    gen = torch.Generator(device=DEV).manual_seed(51 + m)
    d = torch.randn(m, K, device=DEV, generator=gen) * 2
    w = torch.randn(F_, K, device=DEV, generator=gen) * 0.1
    x = torch.randn(m, ldx, device=DEV, generator=gen)[:, :F_]
    mean, invstd = x.mean(0), (x.var(0, unbiased=False) + 1e-5).rsqrt()
    bw = torch.randn(F_, device=DEV, generator=gen) if affine else None
    bb = torch.randn(F_, device=DEV, generator=gen) * 0.3 if affine else None
    ws = gemm.split(w, 1)
    piece = ws.piece
    assert piece == K and piece <= _C.dh_deferred_max_k()
    frag = _C.halves_split_frag(w, ws.scale, piece)
    sc = _C.halves_scale(d)
    db = _C.halves_split(d, sc, 2, piece)
    heads = [(F_, F_)] + ([(250, 252)] if F_ == 750 else [])
    for b_frag in (False, True):
        for two in ((False, True) if K == 128 else (False,)):
            kw = dict(a2_off=piece, b_frag=b_frag, n=F_)
            if two:
                kw.update(scale_a2=torch.tensor([float(sc[0]) * 64, float(sc[1]) / 64], device=DEV), k_split=64)
            B = frag if b_frag else ws.buf
            tag = (m, K, F_, b_frag, two)
            # ---- the storing launch: dy and its partials
            st = _C.BnBwdStats(x, mean, invstd, bw, bb, relu, p, SEED)
            assert st.fits(m, F_, piece)
            dy = _C.gemm_halves3_nt(db, B, sc, ws.scale, piece, piece, piece, bn=st, **kw)
            # ---- reduce-only: the same partials, nothing stored
            st2 = _C.BnBwdStats(x, mean, invstd, bw, bb, relu, p, SEED)
            st2.part.fill_(SENTINEL), st2.pmax.fill_(SENTINEL)
            C = torch.full((m, F_), SENTINEL, device=DEV)
            rkw = {k: v for k, v in kw.items() if k != "a2_off"}
            _C.gemm_halves3_nt_bn_reduce(db, B, sc, ws.scale, piece, piece, st2, piece, out=C, **rkw)
            assert torch.equal(st2.part, st.part) and torch.equal(st2.pmax, st.pmax), tag
            assert bool((C == SENTINEL).all()), tag
            _C.gemm_halves3_nt_bn_reduce(db, B, sc, ws.scale, piece, piece, st2, piece, **rkw)           # C = NULL
            assert torch.equal(st2.part, st.part) and torch.equal(st2.pmax, st.pmax), tag
            # ---- apply mode against the apply pass over the stored dy, with the same finished sums
            slots = _C.absmax_slots(DEV)
            sg, sgx = st.finish(True, m, slots)
            hscale = _C.halves_scale_from_slots(slots)
            for sums in ((sg, sgx), (None, None)):
                for hD, hDP in heads:
                    width = 2 * (F_ // hD) * hDP
                    for want_dx in (True, False):
                        h_ref = torch.full((m, width), SENTINEL, dtype=torch.float16, device=DEV)
                        h_got = torch.full((m, width), SENTINEL, dtype=torch.float16, device=DEV)
                        dx_ref = torch.full((m, F_), SENTINEL, device=DEV) if want_dx else None
                        dx_got = torch.full((m, F_), SENTINEL, device=DEV) if want_dx else None
                        _C.bn_act_bwd_apply_halves(dy, x, mean, invstd, bw, bb, relu, p, SEED, sums[0], sums[1], m, hscale, h_ref, hD, hDP, out=dx_ref)
                        a_ref, a_got = _C.absmax_slots(DEV), _C.absmax_slots(DEV)
                        _C.bn_act_bwd_apply(dy, x, mean, invstd, bw, bb, relu, p, SEED, sums[0], sums[1], m, absmax=a_ref)
                        _C.gemm_halves3_nt_bn_apply(db, B, sc, ws.scale, piece, piece, st2, piece, sums[0], sums[1], m, out=dx_got, hscale=hscale,
                                                    hout=h_got, hD=hD, hDP=hDP, absmax=a_got, **rkw)
                        sub = tag + (sums[0] is None, hD, want_dx)
                        if want_dx:
                            assert torch.equal(dx_got, dx_ref), sub
                        assert torch.equal(h_got, h_ref), sub
                        assert hDP == hD or bool((h_got[:, hD:hDP] == SENTINEL).all()), sub          # padding columns: untouched
                        assert int(a_got.max()) == int(a_ref.max()) and int(a_ref.max()) > 0, sub
            # fp32 only (no halves operand), into a column range of a wider buffer
            wide_ref, wide_got = torch.full((m, F_ + 10), SENTINEL, device=DEV), torch.full((m, F_ + 10), SENTINEL, device=DEV)
            _C.bn_act_bwd_apply(dy, x, mean, invstd, bw, bb, relu, p, SEED, sg, sgx, m, out=wide_ref[:, 2:2 + F_])
            _C.gemm_halves3_nt_bn_apply(db, B, sc, ws.scale, piece, piece, st2, piece, sg, sgx, m, out=wide_got[:, 2:2 + F_], **rkw)
            assert torch.equal(wide_got, wide_ref), tag


def test_shapes_the_deferred_form_does_not_cover_are_refused():
    """BOT_E_RANGE (-2): a piece width above the bound (the hidden layers' products keep the storing form), and an odd BatchNorm width."""
    gen = torch.Generator(device=DEV).manual_seed(5)
    m = 300
    for K, F_ in ((320, 192), (64, 33)):
        d = torch.randn(m, K, device=DEV, generator=gen)
        w = torch.randn(F_, K, device=DEV, generator=gen)
        x = torch.randn(m, F_ + F_ % 2, device=DEV, generator=gen)[:, :F_]
        ws = gemm.split(w, 1)
        piece = ws.piece
        sc = _C.halves_scale(d)
        db = _C.halves_split(d, sc, 2, piece)
        st = _C.BnBwdStats(x, torch.zeros(F_, device=DEV), torch.ones(F_, device=DEV), None, None, True, 0.0, 0)
        dx = torch.empty(m, F_ + F_ % 2, device=DEV)[:, :F_]
        with pytest.raises(_C.BotKernelError, match=r"rc=-2"):
            _C.gemm_halves3_nt_bn_reduce(db, ws.buf, sc, ws.scale, piece, piece, st, piece)
        with pytest.raises(_C.BotKernelError, match=r"rc=-2"):
            _C.gemm_halves3_nt_bn_apply(db, ws.buf, sc, ws.scale, piece, piece, st, piece, None, None, m, out=dx)
    assert _C.dh_deferred_max_k() == 256 < 1536


def _train_step(model, g, feat, labels):
    model.zero_grad(set_to_none=True)
    torch.manual_seed(99)                                   # the dropout seeds of the step
    logits = model(g, feat)
    loss = F.cross_entropy(logits, labels)
    loss.backward()
    return loss.detach().clone(), logits.detach().clone(), {k: v.grad.detach().clone() for k, v in model.named_parameters()}


def test_layer_stack_is_bit_identical_with_the_switch_on_and_off():
    n, fin, C = 600, 64, 40
    rs, rd = powerlaw_edges(n, 5000, 7)
    g = bot_amd.preprocess(bot_amd.Graph(rs, rd, n).to(DEV))
    saved = gemm.FORCE, fused.FORCE, fused.SKIP_Y, gemm.BN_BYPRODUCT, gemm.DH_DEFERRED
    try:
        gemm.FORCE = fused.FORCE = True
        cfg = dict(ARXIV_GAT, dropout=0.75, input_drop=0.25, attn_drop=0.1)
        torch.manual_seed(3)
        model = bnn.GAT(dim_node=fin, dim_edge=0, dim_output=C, activation=F.relu, **cfg).train().to(DEV)
        gen = torch.Generator().manual_seed(4)
        feat = torch.randn(n, fin, generator=gen).to(DEV)
        labels = torch.randint(0, C, (n,), generator=gen).to(DEV)
        runs, counts = {}, {}
        for name, (deferred, skip_y, byproduct) in dict(on=(True, True, True), off=(False, True, True), stored_y=(True, False, True),
                                                        no_byproduct=(True, True, False)).items():
            gemm.DH_DEFERRED, fused.SKIP_Y, gemm.BN_BYPRODUCT = deferred, skip_y, byproduct
            c0 = gemm.DH_DEFERRED_CALLS
            runs[name] = _train_step(model, g, feat, labels)
            counts[name] = gemm.DH_DEFERRED_CALLS - c0
        assert counts == dict(on=1, off=0, stored_y=0, no_byproduct=0), counts      # the output layer's product, and only under every condition
        (loss1, logits1, grads1), (loss0, logits0, grads0) = runs["on"], runs["off"]
        assert torch.equal(loss1, loss0) and torch.equal(logits1, logits0)
        assert set(grads1) == set(grads0) and len(grads1) > 0
        for k in grads1:
            assert torch.equal(grads1[k], grads0[k]), k
    finally:
        gemm.FORCE, fused.FORCE, fused.SKIP_Y, gemm.BN_BYPRODUCT, gemm.DH_DEFERRED = saved
