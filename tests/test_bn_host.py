"""tests/bn_cases.py held to account on the CPU: the float64 restatement of the BatchNorm + ReLU + dropout passes against
torch.nn.BatchNorm1d + relu autograd in float64 (forward and every gradient), the Philox known answer and the mask's keep rate, the
restated dispatch's form count and the case list's coverage, every premise of the exact regime, the undecided-gate share of every seeded
case, the mutants of the restatement (each must be rejected by a check test_bn_gpu.py applies) and the existing CPU emulation of the
passes (tests/_oracle_backend.py) held to the same restatement at p = 0."""
import numpy as np
import pytest
import torch

from tests import _oracle_backend as OB
from tests import bn_cases as BC
from tests import spmm_cases as SC
from tests.test_sampling_host import philox4x32_10

U = BC.U


def _case(**kw):
    base = dict(n=37, F=10, rx=BC.R0, rdy=BC.R0, rdx=BC.R0, ry=BC.R0, relu=True, affine="wb", p=0.0, off=None, regime="seeded", max=True, evalmode=False,
                hd=None, tag="host")
    base.update(kw)
    return BC.Case(**base)


@pytest.mark.parametrize("n,F,affine", [(37, 10, "wb"), (5, 3, None), (130, 6, "w"), (64, 1, "b")])
def test_restatement_matches_batchnorm1d_autograd(n, F, affine):
    """stats64 + reference (p = 0) is nn.BatchNorm1d (training mode) followed by relu: y, the running statistics, and dx, dweight
    (= sum_gx), dbias (= sum_g) of autograd, all in float64."""
    c = _case(n=n, F=F, affine=affine)
    i = BC.make_inputs(c, 3)
    s = BC.stats64(i.x, i.eps, i.momentum, i.rm, i.rv, 0)
    i.mean, i.invstd = s["mean"], s["invstd"]            # float64 statistics here: the restatement is then the float64 BatchNorm exactly
    i.sum_g = i.sum_gx = None
    r0 = BC.reference(i, want_dx=False)
    i.sum_g, i.sum_gx, i.cinv = r0["sum_g"], r0["sum_gx"], 1.0 / n
    r = BC.reference(i)
    bn = torch.nn.BatchNorm1d(F, eps=float(np.float32(i.eps)), momentum=float(np.float32(i.momentum)), affine=True).double().train()
    with torch.no_grad():
        bn.weight.copy_(i.w.double() if i.w is not None else torch.ones(F))
        bn.bias.copy_(i.b.double() if i.b is not None else torch.zeros(F))
        bn.running_mean.copy_(i.rm.double()), bn.running_var.copy_(i.rv.double())
    x = i.x.double().requires_grad_(True)
    y = torch.relu(bn(x))
    y.backward(i.dy.double())
    tol = dict(rtol=1e-11, atol=1e-11)
    assert torch.allclose(y.detach(), r["y"], **tol)
    if n > 1:
        assert torch.allclose(x.grad, r["dx"], **tol) and torch.allclose(bn.bias.grad, r["sum_g"], **tol) and torch.allclose(bn.weight.grad, r["sum_gx"], **tol)
    assert torch.allclose(bn.running_mean, s["rm"], **tol) and torch.allclose(bn.running_var, s["rv"], **tol) and int(bn.num_batches_tracked) == s["nbt"]
    # eval mode: the statistics are constants
    x2 = i.x.double().requires_grad_(True)
    bn.eval()
    with torch.no_grad():
        bn.running_mean.copy_(s["mean"]), bn.running_var.copy_(1.0 / s["invstd"] ** 2 - float(np.float32(i.eps)))
    torch.relu(bn(x2)).backward(i.dy.double())
    assert torch.allclose(x2.grad, r["dx_eval"], rtol=1e-9, atol=1e-9)


def test_philox_known_answer_and_keep_rate():
    assert [hex(int(v)) for v in philox4x32_10(0, np.array([0], dtype=np.uint64))[0]] == ["0x6627e8d5", "0xe169c58d", "0xbc57ac4c", "0x9b00dbd8"]
    for p in (0.3, 0.5, 0.75):
        k = BC.keep_mask(4000, 30, p, 99, 3)
        assert abs(float(k.double().mean()) - (1 - p)) < 4 * (p * (1 - p) / k.numel()) ** 0.5
        assert abs(float(k[:, 29].double().mean()) - (1 - p)) < 5 * (p * (1 - p) / 4000) ** 0.5       # the tail quad's words too
        assert not torch.equal(k, BC.keep_mask(4000, 30, p, 99, None)) and not torch.equal(k, BC.keep_mask(4000, 30, p, 100, 3))
    assert BC.keep_mask(5, 7, 0.0, 1).all()
    # element (r, c) is a function of (r, c, ceil(F / 4)) only: the same block serves F = 29 ... 32
    assert torch.equal(BC.keep_mask(50, 30, 0.5, 7)[:, :29], BC.keep_mask(50, 29, 0.5, 7))
    assert BC.drop_factor(0.5) == 2.0 and BC.drop_factor(0.75) == 4.0 and BC.drop_factor(0.0) == 1.0
    assert BC.drop_factor(0.3) == float(np.float32(1.0) / (np.float32(1.0) - np.float32(0.3)))


def test_dispatch_form_count_and_case_coverage():
    """61 launch forms from the restated dispatch; vec 2 is unreachable; the case list reaches every form and every promised value."""
    assert len(BC.all_forms()) == BC.N_FORMS == 61
    assert BC.unreachable_vec2()
    assert not any("<2>" in s for s in BC.all_forms())
    n_cases, n_stage = BC.assert_coverage()
    assert n_cases == len(BC.cases()) and n_stage == len(BC.stage_cases())
    # the forms by hand, at a few placements
    assert BC.bn_form(8, (8, 8), (0, 0)) == (4, False, (True, True))
    assert BC.bn_form(6, (6, 8), (0, 0)) == (4, True, (False, True))
    assert BC.bn_form(6, (8, 8), (8, 0)) == (4, True, (False, True))
    assert BC.bn_form(6, (7, 8), (0, 0))[:2] == (1, False) and BC.bn_form(6, (6, 6), (4, 0))[:2] == (1, False) and BC.bn_form(5, (8, 8), (0, 0))[:2] == (1, False)
    assert BC.bn_form(8, (8, 8), (0, None)) == (4, False, (True, False))
    assert BC.fwd_form(962, 962, 0, 962, 0, 3)[2] == "rowseg" and BC.fwd_form(1026, 1026, 0, 1026, 0, 3)[2] == "tiled"
    assert BC.fwd_form(750, 752, 0, 750, 0, 2)[0] == "bot::bn_act_fwd_rowseg_kernel<4> rowseg pieces=2 quad wx=1 wy=0"
    assert BC.apply_name(6, 6, 4, 6, 0, 6, 0, True) == "bot::bn_act_bwd_apply_kernel<1> halves"
    assert [BC.nblk_of(n) for n in (1, 4, 5, 1024, 1025, 8193)] == [1, 1, 2, 256, 256, 256]
    assert [BC.rows_per_thread(n) for n in (1, 1024, 1025, 4096, 4097, 8193)] == [1, 1, 2, 4, 5, 9]


def test_exact_premises_and_undecided_share():
    """Every exact case satisfies the premises of bit equality; every seeded case leaves at most 1e-4 of its entries undecided."""
    worst = 0.0
    for k, c in enumerate(BC.cases()):
        i = BC.make_inputs(c, k)
        r = BC.reference(i)
        if c.regime == "exact":
            BC.assert_exact(i, r)
            assert not bool(r["und"].any())
        else:
            share = BC.undecided_share(i, r)
            worst = max(worst, share)
            assert share <= BC.UNDECIDED_SHARE, (c, share)
    print("largest undecided share", worst)
    x, mean, invstd, w, b, share = BC.gate_inputs()
    assert share >= 0.05 and x.shape == (129, 40)


def _perfect(i, r):
    """What a correct device returns in the exact regime: the restatement's float32 values and halves bits."""
    return {k: r[k].float() for k in ("y", "sum_g", "sum_gx", "dx", "gmax")}


@pytest.mark.parametrize("mutant", sorted(BC.MUTANTS))
def test_mutants_are_rejected(mutant):
    """Each mutant of the restatement differs from the unmutated one in a quantity test_bn_gpu.py compares bit for bit."""
    c = _case(n=37, F=18, regime="exact", p=0.5, off=2, hd=(6, 8))
    i = BC.make_inputs(c, 11)
    good = BC.reference(i)
    BC.assert_exact(i, good)
    assert bool((good["pre"] == 0).any()), "the >= 0 mutant needs entries on the boundary"
    got = _perfect(i, good)
    if mutant == 3:
        a, b = BC.stats64(i.x, i.eps, i.momentum, i.rm, i.rv, 0), BC.stats64(i.x, i.eps, i.momentum, i.rm, i.rv, 0, mutant=3)
        assert bool(((a["rv"] - b["rv"]).abs() > a["e_rv"] + b["e_rv"]).all())
        return
    if mutant == 8:      # (exact-regime values have fewer than 11 bits: their second half is zero; the seeded decode check is what rejects this one)
        y32 = BC.reference(BC.make_inputs(c._replace(regime="seeded"), 11))["y"].float()
        buf = BC.fwd_halves_expected(y32, 64.0, c.F, 64, 2, mutant=8)
        assert not torch.equal(buf, BC.fwd_halves_expected(y32, 64.0, c.F, 64, 2))
        bad = []
        BC.check_values(bad, None, "halves", False, BC.fwd_halves_decode(buf, 64.0, c.F, 64, 2), y32.double(), BC.halves_bound(y32.double(), torch.zeros(()), 64.0))
        assert bad
        return
    if mutant == 9:
        dx32 = good["dx"].float()
        assert not torch.equal(BC.heads_expected(dx32, 64.0, c.F, 6, 8), BC.heads_expected(dx32, 64.0, c.F, 6, 8, mutant=9))
        return
    ref = BC.reference(i, mutant=mutant)
    bad = []
    for k in ("y", "sum_g", "sum_gx", "dx"):
        BC.check_values(bad, None, k, True, got[k], ref[k], None)
    assert bad, BC.MUTANTS[mutant]
    if mutant in (1, 2):
        assert not torch.equal(good["keep"], ref["keep"])
        assert not BC.check_mask(got["y"], ref["keep"] & (ref["pre"] > 0))


def test_checks_accept_the_restatement_itself():
    """The other side of the mutants: the unmutated restatement passes its own checks, exact and seeded."""
    for regime in ("exact", "seeded"):
        c = _case(n=130, F=18, regime=regime, p=0.5)
        i = BC.make_inputs(c, 4)
        r = BC.reference(i)
        bad = []
        for k, e in (("y", "e_y"), ("sum_g", "e_sum_g"), ("sum_gx", "e_sum_gx"), ("dx", "e_dx")):
            BC.check_values(bad, None, k, regime == "exact", r[k].float(), r[k], r[e] + U * r[k].abs())
        assert not bad, bad
        y32 = r["y"].float()
        buf = BC.fwd_halves_expected(y32, 16.0, c.F, 64, 3)
        assert float((BC.fwd_halves_decode(buf, 16.0, c.F, 64, 3) - y32.double()).abs().max()) <= float(BC.halves_bound(y32.double(), torch.zeros(()), 16.0).max())
        hb = BC.heads_expected(y32, 16.0, c.F, 6, 8)
        assert torch.equal(hb != SC.SENTINEL16, BC.heads_mask(c.n, c.F, 6, 8))
        assert float((BC.heads_decode(hb, 16.0, c.F, 6, 8) - y32.double()).abs().max()) <= float(BC.halves_bound(y32.double(), torch.zeros(()), 16.0).max())


@pytest.mark.parametrize("regime", ("exact", "seeded"))
def test_oracle_backend_emulation_against_the_restatement(regime):
    """tests/_oracle_backend.py's float32 emulation of the passes (what the CPU suite runs in place of the kernels) at p = 0: bit for
    bit in the exact regime, under the bounds on seeded inputs."""
    for affine in BC.AFFINE:
        c = _case(n=130, F=18, regime=regime, affine=affine)
        i = BC.make_inputs(c, 8)
        r = BC.reference(i)
        exact = regime == "exact"
        bad = []
        y = OB.bn_act_fwd(i.x, i.mean, i.invstd, i.w, i.b, True, 0.0, 1)
        BC.check_values(bad, None, "y", exact, y, r["y"], r["e_y"])
        sg, sgx, mx = OB.bn_act_bwd_reduce(i.dy, i.x, i.mean, i.invstd, i.w, i.b, True, 0.0, 1, want_max=True)
        n_terms = c.n * U                                      # torch's float32 column sum: at most n roundings on any path
        BC.check_values(bad, None, "sum_g", exact, sg, r["sum_g"], r["e_sum_g"] + n_terms * r["g"].abs().sum(0))
        BC.check_values(bad, None, "sum_gx", exact, sgx, r["sum_gx"], r["e_sum_gx"] + n_terms * r["gx"].abs().sum(0))
        BC.check_values(bad, None, "gmax", exact, mx[0], r["gmax"], BC.gamma(1) * r["gmax_alt"], alt=r["gmax_alt"])
        BC.check_values(bad, None, "xmax", exact, mx[1], r["xmax"], BC.gamma(2) * r["xmax"])
        dx = OB.bn_act_bwd_apply(i.dy, i.x, i.mean, i.invstd, i.w, i.b, True, 0.0, 1, i.sum_g, i.sum_gx, i.total_count)
        BC.check_values(bad, None, "dx", exact, dx, r["dx"], r["e_dx"] + 2 * U * r["dx"].abs(), alt=r["dx_alt"])
        dxe = OB.bn_act_bwd_apply(i.dy, i.x, i.mean, i.invstd, i.w, i.b, True, 0.0, 1, None, None, i.total_count)
        BC.check_values(bad, None, "dx eval", exact, dxe, r["dx_eval"], r["e_dx_eval"], alt=r["dx_eval_alt"])
        s = BC.stats64(i.x, i.eps, i.momentum, i.rm, i.rv, 0)
        rm, rv = i.rm.clone(), i.rv.clone()
        mean, invstd = OB.bn_stats(i.x, i.eps, i.momentum, rm, rv)
        wide = c.n * U                                          # the emulation sums without a pivot, n roundings
        BC.check_values(bad, None, "mean", False, mean, s["mean"], s["e_mean"] + wide * i.x.double().abs().mean(0))
        BC.check_values(bad, None, "invstd", False, invstd, s["invstd"], s["e_invstd"] + wide * s["invstd"])
        BC.check_values(bad, None, "rv", False, rv, s["rv"], s["e_rv"] + wide * s["rv"].abs())
        assert not bad, (affine, bad)
