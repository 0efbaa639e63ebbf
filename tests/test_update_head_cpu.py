"""CPU proof of tests/update_head_helpers.py, the oracle tests/test_hip_update_head.py holds the loss, optimiser and GAE
kernels to: the float64 references agree with torch's own operators (cross_entropy with ignore_index, minimum / clamp
autograd, Adam + clip_grad_norm_) and with the kernel's closed-form gradient; the cases realise the branches and edges they
claim; and every mutant of a reference -- one wrong line each -- falls outside the bound the GPU file uses (MARGIN x e32),
on every case it applies to."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import update_head_helpers as H
from oracle import keisei_oracle as orc

SMALL_A = (1, 31, 33, 257)
POLICY_IDS = [f"A{A}-s{s}" for A, s in H.POLICY_CASES]
VALUE_IDS = [f"B{B}-{k}" for B, k in H.VALUE_CASES]


# ------------------------------------------------------------------------------------------------ references vs torch

@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("A", SMALL_A)
def test_policy_reference_agrees_with_torch_and_the_closed_form(A, dt):
    """new_lp / entropy = the oracle's masked_policy_terms, the row losses = clip_surrogate, and autograd's dlogits = the
    closed form the kernel evaluates: g_j = p_j (w_e (lp_j + H) - dnlp) + [j = a] dnlp, dnlp = -w_p r dmin/dr, where
    dmin/dr is adv on the unclipped branch and 0 on the clipped one (torch.minimum / clamp autograd)."""
    for scale in H.POLICY_SCALES:
        case = H.policy_case(A, scale)
        ref = H.policy_ref(case, dt)
        legal, act = case.legal[case.idx], case.actions[case.idx]
        old, adv = case.old_lp[case.idx].to(dt), case.adv[case.idx].to(dt)
        nlp, ent = orc.masked_policy_terms(case.logits.to(dt), legal, act)
        assert torch.equal(nlp, ref["new_lp"])
        tol = 1e-12 if dt == torch.float64 else 2e-6
        assert abs(float(ent) - float(ref["rowent"].mean())) <= tol * max(1.0, abs(float(ent)))
        assert abs(float(orc.clip_surrogate(nlp, old, adv, H.EPS)) - float(ref["rowloss"].mean())) <= tol * 4
        lp = torch.log_softmax(case.logits.to(dt).masked_fill(~legal, float("-inf")), dim=-1)
        p = lp.exp()
        r = torch.exp(nlp - old)
        s1, s2 = r * adv, r.clamp(1 - H.EPS, 1 + H.EPS) * adv
        inrange = (r >= 1 - H.EPS) & (r <= 1 + H.EPS)
        gr = torch.where(s1 < s2, adv, torch.where(s1 > s2, adv * inrange, 0.5 * adv + 0.5 * adv * inrange))
        dnlp = -gr * r * (H.W.lambda_policy / H.PB)
        g = p * (H.W.entropy_coeff / H.PB * (lp.masked_fill(~legal, 0.0) + ref["rowent"][:, None]) - dnlp[:, None])
        g[torch.arange(H.PB), act] += dnlp * legal[torch.arange(H.PB), act]
        g = g.masked_fill(~legal, 0.0)
        scale_g = max(float(ref["dlogits"].abs().max()), 1e-30)
        assert float((g - ref["dlogits"]).abs().max()) <= (1e-13 if dt == torch.float64 else 1e-5) * scale_g


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("B,kind", [(63, "mixed"), (65, "mixed"), (1025, "ignored"), (1025, "valid")])
def test_value_reference_agrees_with_torch(B, kind, dt):
    case = H.value_case(B, kind)
    ref = H.value_ref(case, dt, 0)
    vl, sc = case.vlogits.to(dt).requires_grad_(True), case.score.to(dt).requires_grad_(True)
    cats, tg = case.cats[case.idx], case.targets[case.idx].to(dt)
    ce = orc.wdl_ce(vl, cats)                                     # F.cross_entropy(ignore_index=-1) / the all-ignored 0
    mse = F.mse_loss(sc, tg)
    dv, ds = torch.autograd.grad(H.W.lambda_value * ce + H.W.lambda_score * mse, [vl, sc])
    tol = 1e-12 if dt == torch.float64 else 1e-6
    assert abs(float(ce.detach()) - float(ref["out"][1])) <= tol and abs(float(mse.detach()) - float(ref["out"][2])) <= tol * 4
    assert torch.allclose(dv, ref["dvlogits"], rtol=tol * 10, atol=tol * 1e-3)
    assert torch.allclose(ds, ref["dscore"], rtol=tol * 10, atol=tol * 1e-3)
    if kind == "ignored":
        assert float(ref["out"][1]) == 0.0 and not bool(ref["dvlogits"].any()) and ref["counts"] == (0, 0, 0, 0)
        assert H.value_fractions(ref["counts"]) == [0.0, 0.0, 0.0, 0.0]
    pred = case.vlogits.argmax(dim=1)                             # torch.argmax: the first maximum
    valid = cats >= 0
    assert ref["counts"] == (int(valid.sum()), int((pred == cats)[valid].sum()), int((pred == 0)[valid].sum()),
                             int((pred == 1)[valid].sum()))
    assert pred[:3].tolist() == list(H.TIE_PRED)


def test_value_reference_accumulator_modes():
    case = H.value_case(65, "mixed")
    a0, a1 = H.value_ref(case, torch.float64, 0), H.value_ref(case, torch.float64, 1)
    pl, ce, mse, ent, total = (float(x) for x in a0["out"])
    assert a0["acc"].tolist() == [pl, ce, mse, ent]
    assert a1["acc"].tolist() == [pl, H.W.lambda_value * ce + H.W.lambda_score * mse, 0.0, ent]
    assert abs(total - (pl + 1.5 * ce + 0.02 * mse - 0.01 * ent)) < 1e-14
    assert torch.equal(a0["out"], a1["out"])


@pytest.mark.parametrize("dt", [torch.float32, torch.float64], ids=["f32", "f64"])
def test_adam_reference_agrees_with_torch(dt):
    p0, grads = H.adam_case()
    ref = H.adam_ref(dt=dt)
    params = [torch.nn.Parameter(t.clone().to(dt)) for t in p0]
    opt = torch.optim.Adam(params, lr=H.ADAM_LR, betas=H.ADAM_BETAS)
    for s in range(3):
        for p, g in zip(params, grads[s]):
            p.grad = g.clone().to(dt)
        norm = torch.nn.utils.clip_grad_norm_(params, H.ADAM_MAX_NORM)
        opt.step()
        assert abs(float(norm) - ref["norms"][s]) <= 1e-6 * ref["norms"][s]
        for a, b in zip(params, ref["params"][s]):
            assert float((a.detach() - b).abs().max()) <= 1e-7        # (an update is <= lr = 2e-4 per element)
    assert ref["coefs"][0] < 0.1 and ref["coefs"][1] == 1.0 and 0.5 < ref["coefs"][2] < 1.0
    for i, p in enumerate(params):
        st = opt.state[p]
        assert torch.allclose(st["exp_avg"], ref["m"][i], rtol=1e-5, atol=1e-9)
        assert torch.allclose(st["exp_avg_sq"], ref["v"][i], rtol=1e-5, atol=1e-11)
        assert float(ref["params"][2][i][-1]) != float(p0[i][-1])     # every tensor's last element moves


def test_scaler_rule():
    assert H.scaler_rule(65536.0, 5.0, False) == (32768.0, 0.0)
    assert H.scaler_rule(1024.0, 0.0, True) == (1024.0, 1.0)
    assert H.scaler_rule(1024.0, 1998.0, True) == (1024.0, 1999.0)
    assert H.scaler_rule(1024.0, 1999.0, True) == (2048.0, 0.0)


def test_mask_codec_round_trip():
    for A in (1, 31, 32, 33, 257):
        legal = torch.rand(5, A, generator=torch.Generator().manual_seed(A)) < 0.4
        legal[0] = False; legal[0, A - 1] = True
        bits = H.pack_mask_rows(legal)
        assert bits.shape == (5, (A + 31) // 32) and bits.dtype == torch.int32
        assert torch.equal(H.unpack_mask_rows(bits, A), legal)
        assert int(bits[0, -1].item()) & 0xFFFFFFFF == 1 << ((A - 1) & 31)
        if A > 1:
            assert not torch.equal(H.unpack_mask_rows(bits, A, mutant="bit_order"), legal)


# ------------------------------------------------------------------------------------------------ the case conditions

@pytest.mark.parametrize("A,scale", H.POLICY_CASES, ids=POLICY_IDS)
def test_policy_case_conditions(A, scale):
    count = H.policy_conditions(H.policy_case(A, scale))
    assert sum(count.values()) == 13           # the adv = 0 rows and the ratio-0 row stand apart


@pytest.mark.parametrize("B,kind", H.VALUE_CASES, ids=VALUE_IDS)
def test_value_case_conditions(B, kind):
    H.value_conditions(H.value_case(B, kind))
    H.value_conditions(H.value_case(B, kind, 1))


def test_other_case_conditions():
    assert H.ADAM_TAIL == (True, True, False, True, True, False, True, True, True)
    for T, N in H.GAE_SHAPES:
        lengths = H.gae_case(T, N, False)[5]
        assert lengths.min() == 0 and (N == 1 or lengths.max() == T)
    for n in H.NORMALIZE_N:
        x = H.normalize_case(n)
        assert x.numel() == n and abs(float(x.mean()) - 3.0) < 1.5


# ------------------------------------------------------------------------------------------------ the mutants

@pytest.mark.parametrize("mutant", sorted(H.MUTANTS_POLICY))
@pytest.mark.parametrize("A,scale", H.POLICY_CASES, ids=POLICY_IDS)
def test_policy_mutants_fail_the_bound(A, scale, mutant):
    case = H.policy_case(A, scale)
    ref, e32 = H.policy_refs(A, scale)
    assert H.worst_excess(ref, ref, e32)[0] == 0.0
    r32 = H.policy_ref(case, torch.float32)
    assert H.worst_excess(r32, ref, e32)[0] <= 1.0                # (the fp32 run itself defines e32)
    if not H.MUTANTS_POLICY[mutant](case):
        return
    if mutant == "bit_order":
        legal = H.unpack_mask_rows(H.pack_mask_rows(case.legal), A, mutant="bit_order")
        assert not torch.equal(legal[case.idx], case.legal[case.idx])
        got = H.policy_ref(case, torch.float64, legal=legal)
    elif mutant == "entropy_unscaled":                            # seen through the GPU file's identity scaled = 1024 x unscaled
        got = H.policy_ref(case, torch.float64, mutant=mutant, gscale=H.GSCALE)
        got["dlogits"] = got["dlogits"] / H.GSCALE
    else:
        got = H.policy_ref(case, torch.float64, mutant=mutant)
    worst, name = H.worst_excess(got, ref, e32)
    assert worst > 10 * H.MARGIN, (mutant, case.name, name, worst)


@pytest.mark.parametrize("mutant", sorted(H.MUTANTS_VALUE))
@pytest.mark.parametrize("B,kind", H.VALUE_CASES, ids=VALUE_IDS)
def test_value_mutants_fail_the_bound(B, kind, mutant):
    case = H.value_case(B, kind)
    for use_idx in (True, False):
        for combined in (0, 1):
            ref, e32 = H.value_refs(B, kind, combined, use_idx)
            if not H.MUTANTS_VALUE[mutant](case, use_idx):
                continue
            got = H.value_ref(case, torch.float64, combined, mutant=mutant, use_idx=use_idx)
            if mutant == "tie_last":                              # the counts are held exactly
                assert H.value_fractions(got["counts"]) != H.value_fractions(ref["counts"]), case.name
                continue
            worst, name = H.worst_excess(got, ref, e32)
            assert worst > 10 * H.MARGIN, (mutant, case.name, name, worst)


def test_value_mutants_apply_somewhere():
    # CE over B shows where some but not all rows are valid (every mixed case but B = 1), the tie rule wherever a row counts
    want = {"ce_over_B": len(H.VALUE_B) - 1, "score_no_2": len(H.VALUE_CASES), "tie_last": len(H.VALUE_CASES) - 1}
    for mutant, applies in H.MUTANTS_VALUE.items():
        assert sum(applies(H.value_case(B, kind)) for B, kind in H.VALUE_CASES) == want[mutant], mutant


def test_adam_tail_mutant_fails_exactly_the_tensors_with_a_tail():
    ref = H.adam_ref()
    assert H.adam_mismatch(ref, ref) == []
    bad = H.adam_mismatch(H.adam_ref(mutant="tail_dropped"), ref)
    assert bad == [i for i, tail in enumerate(H.ADAM_TAIL) if tail]


def test_bound_helpers():
    ref = torch.tensor([1.0, -2.0, -math.inf], dtype=torch.float64)
    assert H.e32_of(ref.float(), ref) == H.FLOOR * 2.0            # an exact fp32 run: the floor
    assert H.excess(ref.float(), ref, 1e-6) == 0.0
    assert H.excess(torch.tensor([1.0, -2.0, 0.0]), ref, 1e-6) == math.inf
    assert H.excess(torch.tensor([1.0, math.nan, -math.inf]), ref, 1e-6) == math.inf
    assert abs(H.excess(torch.tensor([1.0, -2.0 + 3e-6, -math.inf], dtype=torch.float64), ref, 1e-6) - 3.0) < 1e-6
    zero = torch.zeros(3, dtype=torch.float64)
    assert H.e32_of(zero.float(), zero) == 0.0 and H.excess(zero.float(), zero, 0.0) == 0.0
    assert H.excess(torch.tensor([0.0, 1e-30, 0.0]), zero, 0.0) == math.inf
    assert np.float32(1 / 3) == np.float32(np.float64(1) / np.float64(3))
