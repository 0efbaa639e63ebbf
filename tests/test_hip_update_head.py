"""The update head on the GPU -- ka_policy_loss, ka_value_loss, ka_policy_ce, ka_masked_softmax, ka_scalar_value
(csrc/loss.hip), ka_normalize_advantages, ka_gae (csrc/gae.hip) and ka_clip_adam_step (csrc/optim.hip) -- against the float64
references of tests/update_head_helpers.py (proved, with their mutants, in tests/test_update_head_cpu.py), at the sizes where
the kernels change path: action counts below one staging pass, inside a mask word and of one action; value batches around
the wave, the 1024-thread stride and beyond; optimiser tensors around the 256-thread stride and the 4096-element chunk.

Bound: per output tensor, MARGIN = 4 x e32, e32 = the distance of the same formula run in float32 torch on the CPU from its
float64 run (floored at 2^-22 of the tensor's largest entry).  Each comparison prints `ratio <kernel> <case> <tensor> <x e32>`
before it asserts.  Identities that hold exactly -- packed = bool masks, index = gathered rows, a power-of-two loss scale,
the GradScaler unscale -- are asserted bit for bit."""
import functools
import math

import numpy as np
import pytest
import torch

import update_head_helpers as H
from keisei_amd import _lib
from oracle import keisei_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")
PATTERN = 0x5A5AA5A5
POLICY_IDS = [f"A{A}-s{s}" for A, s in H.POLICY_CASES]
VALUE_IDS = [f"B{B}-{k}" for B, k in H.VALUE_CASES]


def st():
    return _lib.stream_ptr()


def dev(t):
    return t.contiguous().to(DEV)


def held(kernel, case, got, ref, e32):
    """print every tensor's distance in units of e32, then hold the worst to MARGIN"""
    worst = 0.0
    for k in e32:
        x = H.excess(got[k], ref[k], e32[k])
        print(f"ratio {kernel} {case} {k} {x:.3f} (e32 {e32[k]:.3e})")
        worst = max(worst, x)
    assert worst <= H.MARGIN, (kernel, case, worst)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ ka_policy_loss

def run_policy(case, packed=False, use_idx=True, with_dl=True, gscale=None, logits=None, legal=None, actions=None):
    B, A = H.PB, case.A
    logits = case.logits if logits is None else logits
    legal = case.legal if legal is None else legal
    actions = case.actions if actions is None else actions
    old, adv = case.old_lp, case.adv
    index = dev(case.idx) if use_idx else None
    if not use_idx:                              # the same minibatch with the per-sample data gathered beforehand
        legal, actions, old, adv = legal[case.idx], actions[case.idx], old[case.idx], adv[case.idx]
    masks, words = dev(legal), 0
    if packed:
        words = (A + 31) // 32
        bits = torch.full((legal.shape[0], words), -1, dtype=torch.int32, device=DEV)
        _lib.call("ka_pack_mask_bits", masks, bits, legal.shape[0], A, st())
        assert torch.equal(bits.cpu(), H.pack_mask_rows(legal))
        masks = bits
    guard = torch.full((B + 2, A), PATTERN, dtype=torch.int32, device=DEV)
    dl = guard.view(torch.float32)[1:B + 1]
    dl.fill_(NAN)
    nlp, rl, re = (torch.full((B,), NAN, device=DEV) for _ in range(3))
    flags = torch.zeros(2, dtype=torch.int32, device=DEV)
    gs = None if gscale is None else torch.tensor([gscale], device=DEV)
    _lib.call("ka_policy_loss", dev(logits), masks, dev(actions), dev(old), dev(adv), index, dl if with_dl else None, nlp, rl,
              re, flags, gs, H.EPS, H.W.lambda_policy / B, H.W.entropy_coeff / B, B, A, words, st())
    torch.cuda.synchronize()
    assert bool((guard[0] == PATTERN).all()) and bool((guard[B + 1] == PATTERN).all())
    out = {"new_lp": nlp.cpu(), "rowloss": rl.cpu(), "rowent": re.cpu(), "flags": flags.cpu().tolist()}
    if with_dl:
        out["dlogits"] = dl.cpu().clone()
    else:
        assert bool(torch.isnan(dl).all())
    return out


ROWS = ("new_lp", "rowloss", "rowent")


@pytest.mark.parametrize("A,scale", H.POLICY_CASES, ids=POLICY_IDS)
def test_policy_loss_against_fp64(A, scale):
    case = H.policy_case(A, scale)
    ref, e32 = H.policy_refs(A, scale)
    legal = case.legal[case.idx]
    runs = {(p, i): run_policy(case, packed=p, use_idx=i) for p in (False, True) for i in (True, False)}
    base = runs[False, True]
    for key, got in runs.items():
        assert got["flags"] == [0, 0], key
        for k in ROWS + ("dlogits",):            # every element written
            assert not bool(torch.isnan(got[k]).any()), (key, k)
        assert bool(torch.isfinite(got["dlogits"]).all())
        held("policy_loss", f"{case.name}/{'packed' if key[0] else 'bool'}/{'idx' if key[1] else 'gathered'}", got, ref, e32)
        assert bool((got["dlogits"][~legal] == 0).all())
        if A > 1:
            assert bool((got["dlogits"][H.SINGLE] == 0).all()) and float(got["rowent"][H.SINGLE]) == 0.0
        for k in ROWS + ("dlogits",):            # packed = bool, index = gathered: the same arithmetic, the same bits
            assert same_bits(got[k], base[k]), (key, k)
    nodl = run_policy(case, with_dl=False)
    assert nodl["flags"] == [0, 0]
    for k in ROWS:
        assert same_bits(nodl[k], base[k]), k
    # a power-of-two loss scale: the kernel multiplies the finished gradient by it, so the result is the unscaled one times the
    # scale to the bit -- also where a probability times a weight underflows to a subnormal
    scaled = run_policy(case, gscale=H.GSCALE)
    for k in ROWS:
        assert same_bits(scaled[k], base[k]), k
    diff = scaled["dlogits"] != H.GSCALE * base["dlogits"]
    print(f"gscale policy_loss {case.name}: {int(diff.sum())} of {diff.numel()} elements differ from {H.GSCALE:g} x unscaled"
          + (f", the largest of them {float(base['dlogits'][diff].abs().max()):.3e} unscaled" if bool(diff.any()) else ""))
    assert same_bits(scaled["dlogits"], H.GSCALE * base["dlogits"])


@pytest.mark.parametrize("A,scale", [(33, 3), (11259, 3)], ids=["A33", "A11259"])
def test_policy_loss_flags_leave_the_other_rows_alone(A, scale):
    case = H.policy_case(A, scale)
    base = run_policy(case)
    k = 2                                        # the row that is spoiled; its sample is fetched by no other row
    s = int(case.idx[k])
    others = torch.tensor([b for b in range(H.PB) if int(case.idx[b]) != s])
    assert others.numel() == H.PB - 1

    def unchanged(got):
        for name in ROWS + ("dlogits",):
            assert same_bits(got[name][others], base[name][others]), name

    logits = case.logits.clone()
    logits[k, int((~case.legal[s]).nonzero()[0])] = NAN          # a NaN the mask hides is still a NaN from the model
    got = run_policy(case, logits=logits)
    assert got["flags"] == [1, 0]
    unchanged(got)
    for bad in (A, -1):
        actions = case.actions.clone()
        actions[s] = bad
        got = run_policy(case, actions=actions)
        assert got["flags"] == [0, 2], bad
        unchanged(got)
    legal = case.legal.clone()
    legal[s] = False
    got = run_policy(case, legal=legal, packed=True)
    assert got["flags"] == [0, 1]
    unchanged(got)
    assert base["flags"] == [0, 0]


def test_policy_loss_refuses_a_row_beyond_the_lds():
    A, B = 14000, H.PB
    outs = [torch.full((B,), NAN, device=DEV) for _ in range(3)]
    dl = torch.full((B, A), NAN, device=DEV)
    flags = torch.zeros(2, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.KeiseiHipError, match="too large for the LDS row"):
        _lib.call("ka_policy_loss", torch.zeros(B, A, device=DEV), torch.ones(B, A, dtype=torch.bool, device=DEV),
                  torch.zeros(B, dtype=torch.int64, device=DEV), torch.zeros(B, device=DEV), torch.ones(B, device=DEV), None, dl,
                  *outs, flags, None, H.EPS, 1.0 / B, 0.01 / B, B, A, 0, st())
    torch.cuda.synchronize()
    assert bool(torch.isnan(dl).all()) and all(bool(torch.isnan(t).all()) for t in outs) and flags.cpu().tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------ ka_value_loss

def run_value(case, combined, use_idx=True, gscale=None, grads=True, acc=None):
    B = case.B
    dv = torch.full((B, 3), NAN, device=DEV) if grads else None
    ds = torch.full((B,), NAN, device=DEV) if grads else None
    out = torch.full((9,), NAN, device=DEV)
    acc = torch.zeros(4, device=DEV) if acc is None else acc
    gs = None if gscale is None else torch.tensor([gscale], device=DEV)
    _lib.call("ka_value_loss", dev(case.vlogits), dev(case.score), dev(case.cats), dev(case.targets),
              dev(case.idx) if use_idx else None, dev(case.rowloss), dev(case.rowent), dv, ds, out, acc, gs, H.W.lambda_policy,
              H.W.lambda_value, H.W.lambda_score, H.W.entropy_coeff, combined, B, st())
    torch.cuda.synchronize()
    o = out.cpu()
    got = {"out": o[:5].clone(), "tail": o[5:].tolist(), "raw": o, "acc": acc.cpu().clone(), "acc_dev": acc}
    if grads:
        got["dvlogits"], got["dscore"] = dv.cpu(), ds.cpu()
    return got


@pytest.mark.parametrize("B,kind", H.VALUE_CASES, ids=VALUE_IDS)
def test_value_loss_against_fp64(B, kind):
    case, partner = H.value_case(B, kind), H.value_case(B, kind, 1)
    for use_idx in (True, False):
        for combined in (0, 1):
            ref, e32 = H.value_refs(B, kind, combined, use_idx)
            tag = f"{case.name}/{'idx' if use_idx else 'identity'}/metric{combined}"
            got = run_value(case, combined, use_idx)
            assert not any(bool(torch.isnan(got[k]).any()) for k in ("raw", "dvlogits", "dscore"))
            held("value_loss", tag, got, ref, e32)
            assert got["tail"] == H.value_fractions(ref["counts"]), (tag, got["tail"], ref["counts"])
            if kind == "ignored":
                assert float(got["out"][1]) == 0.0 and not bool(got["dvlogits"].any()) and got["tail"] == [0.0] * 4
            # the running sums over two calls: this minibatch, then its partner
            ref2, _ = H.value_refs(B, kind, combined, use_idx, 1.0, 1)
            sum32 = (H.value_ref(case, torch.float32, combined, use_idx=use_idx)["acc"]
                     + H.value_ref(partner, torch.float32, combined, use_idx=use_idx)["acc"])
            sum64 = ref["acc"] + ref2["acc"]
            both = run_value(partner, combined, use_idx, acc=got["acc_dev"])
            held("value_loss", tag + "/two-calls", {"acc": both["acc"]}, {"acc": sum64}, {"acc": H.e32_of(sum32, sum64)})
            if combined:
                assert float(both["acc"][2]) == 0.0
            nograd = run_value(case, combined, use_idx, grads=False)
            assert same_bits(nograd["raw"], got["raw"]) and same_bits(nograd["acc"], got["acc"])
            scaled = run_value(case, combined, use_idx, gscale=H.GSCALE)
            assert same_bits(scaled["raw"], got["raw"])
            assert same_bits(scaled["dvlogits"], H.GSCALE * got["dvlogits"]) and same_bits(scaled["dscore"], H.GSCALE * got["dscore"])


# ------------------------------------------------------------------------------------------------ the small kernels

@pytest.mark.parametrize("A", H.POLICY_A)
def test_policy_ce_against_fp64(A):
    case = H.policy_case(A, 3)
    ref, e32 = H.with_e32(H.policy_ce_ref, case)
    B = H.PB
    dl, rl = torch.full((B, A), NAN, device=DEV), torch.full((B,), NAN, device=DEV)
    flags = torch.zeros(2, dtype=torch.int32, device=DEV)
    _lib.call("ka_policy_ce", dev(case.logits), dev(case.actions), dev(case.idx), dl, rl, flags, None, H.W.lambda_policy / B, B, A, st())
    torch.cuda.synchronize()
    assert flags.cpu().tolist() == [0, 0]
    held("policy_ce", case.name, {"rowloss": rl.cpu(), "dlogits": dl.cpu()}, ref, e32)


@pytest.mark.parametrize("A", H.POLICY_A)
def test_masked_softmax_against_fp64(A):
    case = H.policy_case(A, 3)
    ref, e32 = H.with_e32(H.masked_softmax_ref, case)
    legal = case.legal[case.idx]
    B = H.PB
    probs = torch.full((B, A), NAN, device=DEV)
    nlegal = torch.full((B,), -1, dtype=torch.int32, device=DEV)
    flags = torch.zeros(2, dtype=torch.int32, device=DEV)
    _lib.call("ka_masked_softmax", dev(case.logits), dev(legal), probs, nlegal, flags, B, A, 0, st())
    torch.cuda.synchronize()
    assert flags.cpu().tolist() == [0, 0] and torch.equal(nlegal.cpu().long(), legal.sum(dim=1))
    held("masked_softmax", case.name, {"probs": probs.cpu()}, ref, e32)
    assert bool((probs.cpu()[~legal] == 0).all())


@pytest.mark.parametrize("B", [1, 255, 257])
def test_scalar_value_against_fp64(B):
    case = H.value_case(B)
    ref, e32 = H.with_e32(H.scalar_value_ref, case, 0.1)
    out = torch.full((B,), NAN, device=DEV)
    _lib.call("ka_scalar_value", dev(case.vlogits), dev(3.0 * case.score), 0.1, out, B, st())
    torch.cuda.synchronize()
    held("scalar_value", case.name, {"value": out.cpu()}, ref, e32)


@pytest.mark.parametrize("n", H.NORMALIZE_N)
def test_normalize_advantages_against_fp64(n):
    x = H.normalize_case(n)
    ref, e32 = H.with_e32(H.normalize_ref, x)
    out = torch.full((n,), NAN, device=DEV)
    _lib.call("ka_normalize_advantages", dev(x), out, n, st())
    torch.cuda.synchronize()
    held("normalize_advantages", f"n{n}", {"out": out.cpu()}, ref, e32)


@pytest.mark.parametrize("f64", [False, True], ids=["f32", "f64"])
@pytest.mark.parametrize("T,N", H.GAE_SHAPES)
def test_gae_small_grids_bit_exact(T, N, f64):
    r, v, term, nv, ov, lengths = H.gae_case(T, N, f64)
    assert lengths.min() == 0 and (N == 1 or lengths.max() == T)
    tt = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    for use_ov in (False, True):
        for use_len in (False, True):
            ref = orc.gae_grid(r, v, term, nv, 0.99, 0.95, override=ov if use_ov else None, lengths=lengths if use_len else None)
            adv = torch.full((T, N), NAN, dtype=torch.float64 if f64 else torch.float32, device=DEV)
            _lib.call("ka_gae", tt(r), tt(v), tt(term), tt(nv), tt(ov) if use_ov else None, tt(lengths) if use_len else None,
                      adv, T, N, 0.99, 0.95, int(f64), st())
            got = adv.cpu().numpy()
            assert not np.isnan(got).any()
            # cells past an environment's length are padding; a length of 0 is walked as a length of 1 by both sides
            valid = np.arange(T)[:, None] < np.maximum(lengths, 1)[None, :] if use_len else np.ones((T, N), dtype=bool)
            assert np.array_equal(got[valid], ref[valid]), (use_ov, use_len)


# ------------------------------------------------------------------------------------------------ ka_clip_adam_step

class AdamRig:
    """the odd-sized table on the device, with the block map ka_clip_adam_step walks"""

    def __init__(self):
        p0, self.grads_cpu = H.adam_case()
        self.params = [dev(t.clone()) for t in p0]
        self.grads = [torch.zeros_like(p) for p in self.params]
        self.ms, self.vs = [torch.zeros_like(p) for p in self.params], [torch.zeros_like(p) for p in self.params]
        chunk = _lib.query("ka_adam_chunk")
        assert chunk == 4096
        recs, bt, bo = [], [], []
        for i, p in enumerate(self.params):
            recs += [p.data_ptr(), self.grads[i].data_ptr(), self.ms[i].data_ptr(), self.vs[i].data_ptr(), p.numel()]
            for off in range(0, p.numel(), chunk):
                bt.append(i); bo.append(off)
        self.nb = len(bt)
        self.tab = torch.tensor(recs, dtype=torch.int64, device=DEV)
        self.bt, self.bo = torch.tensor(bt, dtype=torch.int32, device=DEV), torch.tensor(bo, dtype=torch.int64, device=DEV)
        self.partial = torch.empty(self.nb, dtype=torch.float64, device=DEV)
        self.ctl, self.step, self.acc = torch.zeros(4, device=DEV), torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)

    def load(self, s, mul=1.0):
        for gd, gc in zip(self.grads, self.grads_cpu[s]):
            gd.copy_(gc * mul)

    def launch(self, scaler=None, flags=None):
        _lib.call("ka_clip_adam_step", self.tab, self.bt, self.bo, self.nb, self.partial, self.ctl, self.step, scaler, flags,
                  self.acc, H.ADAM_MAX_NORM, H.ADAM_LR, *H.ADAM_BETAS, 1e-8, st())
        torch.cuda.synchronize()
        return self.ctl.cpu().tolist()

    def state(self):
        return [[t.cpu().clone() for t in ts] for ts in (self.params, self.ms, self.vs)]

    def three_steps(self, mul=1.0, scaler=None):
        got = {"params": [], "ctl": []}
        for s in range(3):
            self.load(s, mul)
            got["ctl"].append(self.launch(scaler))
            got["params"].append([p.cpu().clone() for p in self.params])
        got["m"], got["v"] = [t.cpu().clone() for t in self.ms], [t.cpu().clone() for t in self.vs]
        got["acc"], got["step"] = float(self.acc), float(self.step)
        return got


@functools.lru_cache(maxsize=None)
def adam_plain():
    return AdamRig().three_steps()


def test_clip_adam_odd_sizes_against_reference():
    ref, got = H.adam_ref(), adam_plain()
    p0 = H.adam_case()[0]
    for s in range(3):
        norm, coef, skip = got["ctl"][s][:3]
        print(f"adam step {s}: norm {norm:.7g} (ref {ref['norms'][s]:.7g}), coef {coef:.7g} (ref {ref['coefs'][s]:.7g})")
        assert abs(norm - ref["norms"][s]) <= 1e-5 * ref["norms"][s]
        assert abs(coef - ref["coefs"][s]) <= 1e-5 * ref["coefs"][s] and skip == 0.0
    assert H.adam_mismatch(got, ref) == []
    assert abs(got["acc"] - sum(ref["norms"])) <= 1e-5 * sum(ref["norms"]) and got["step"] == 3.0
    for i, n in enumerate(H.ADAM_SIZES):         # the last element of every tensor has moved, in every step
        last = [float(p0[i][-1])] + [float(got["params"][s][i][-1]) for s in range(3)]
        assert len(set(last)) == 4, (n, last)
        assert float(got["m"][i][-1]) != 0.0 and float(got["v"][i][-1]) != 0.0


def test_clip_adam_unscale_is_exact():
    """gradients x 2^10 under a scale of 2^10: the double sum of squares, its root, the division and g * (coef / scale) all
    scale exactly, so weights, moments and the norm are the unscaled run's to the bit; three clean steps count up"""
    plain = adam_plain()
    scaler = torch.tensor([H.GSCALE, 0.0], device=DEV)
    got = AdamRig().three_steps(mul=H.GSCALE, scaler=scaler)
    for s in range(3):
        assert got["ctl"][s][0] == plain["ctl"][s][0] and got["ctl"][s][2] == 0.0
        assert got["ctl"][s][1] * H.GSCALE == plain["ctl"][s][1]
        for a, b in zip(got["params"][s], plain["params"][s]):
            assert same_bits(a, b), s
    for k in ("m", "v"):
        for a, b in zip(got[k], plain[k]):
            assert same_bits(a, b), k
    assert scaler.cpu().tolist() == [H.GSCALE, 3.0] and got["step"] == 3.0 and got["acc"] == plain["acc"]


def test_clip_adam_scaler_growth_nan_and_guard():
    plain = adam_plain()
    # growth at the interval: the step itself is applied
    rig = AdamRig()
    scaler = torch.tensor([H.GSCALE, 1999.0], device=DEV)
    rig.load(0, H.GSCALE)
    ctl = rig.launch(scaler)
    assert scaler.cpu().tolist() == list(H.scaler_rule(H.GSCALE, 1999.0, True)) == [2 * H.GSCALE, 0.0]
    assert ctl[2] == 0.0 and float(rig.step) == 1.0
    for a, b in zip(rig.params, plain["params"][0]):
        assert same_bits(a.cpu(), b)
    # a NaN (not inf) gradient: skipped, nothing touched, the scale backs off
    before = rig.state()
    rig.load(1, 2 * H.GSCALE)
    rig.grads[3][5] = NAN
    scaler = torch.tensor([2 * H.GSCALE, 7.0], device=DEV)
    ctl = rig.launch(scaler)
    assert ctl[2] == 1.0 and math.isnan(ctl[0]) and float(rig.step) == 1.0
    assert scaler.cpu().tolist() == list(H.scaler_rule(2 * H.GSCALE, 7.0, False)) == [H.GSCALE, 0.0]
    for old, new in zip(before, rig.state()):
        assert all(same_bits(a, b) for a, b in zip(old, new))
    # a guard flag in flags[0]: skipped as well, but the norm is finite and the tracker advances
    rig.load(1, H.GSCALE)
    scaler = torch.tensor([H.GSCALE, 7.0], device=DEV)
    flags = torch.tensor([1, 0], dtype=torch.int32, device=DEV)
    ctl = rig.launch(scaler, flags)
    assert ctl[2] == 1.0 and ctl[0] == plain["ctl"][1][0] and float(rig.step) == 1.0
    assert scaler.cpu().tolist() == list(H.scaler_rule(H.GSCALE, 7.0, True)) == [H.GSCALE, 8.0]
    for old, new in zip(before, rig.state()):
        assert all(same_bits(a, b) for a, b in zip(old, new))
    # and without the flag the same gradients go through
    ctl = rig.launch(scaler, torch.zeros(2, dtype=torch.int32, device=DEV))
    assert ctl[2] == 0.0 and float(rig.step) == 2.0 and scaler.cpu().tolist() == [H.GSCALE, 9.0]
    for a, b in zip(rig.params, plain["params"][1]):
        assert same_bits(a.cpu(), b)
