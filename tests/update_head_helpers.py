"""Shared by tests/test_update_head_cpu.py and tests/test_hip_update_head.py: the cases and the float64 references of the
update head -- ka_policy_loss / ka_value_loss (csrc/loss.hip), ka_clip_adam_step (csrc/optim.hip), ka_normalize_advantages
and ka_gae (csrc/gae.hip) -- the packed legal-mask codec, the GradScaler rule and the error bound.  No GPU in here.

The references are torch autograd in float64 on the CPU, written in the style of oracle/keisei_oracle.py (and reusing it
where it fits); run in float32 the SAME formulas give `e32`, the distance a correct fp32 evaluation keeps from float64,
and the kernels are held to MARGIN x e32 per output tensor (e32_of / excess).  The references take `mutant=`: one wrong
line each, the mistakes a kernel could make without crashing; the CPU file shows each of them outside the bound.

Policy cases: B = 16 logits rows, S = 24 per-sample rows fetched through `idx` (the logits row stays b), 15 distinct
samples -- rows 13 and 14 share one.  Row by row (TABLE) the stored old_log_probs are filled from the float64 new_log_prob
so that ratio x advantage realises every branch of the clipped surrogate at least twice, 0.01 away from 1 +- eps; row
SINGLE has one legal action (entropy 0, gradient exactly 0), row ALL has every action legal and has chosen the last one,
row LAST has the chosen action and A - 1 legal, row ILLEGAL has chosen an illegal action (new_log_prob -inf, ratio 0,
gradient 0), every other row ~5 % legal.  A = 1 admits none of the special masks (its one action is legal everywhere)."""
import functools
import math
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from oracle import keisei_oracle as orc

MARGIN = 4.0                                     # the kernels must lie within MARGIN x e32 of float64
FLOOR = 2.0 ** -22                               # e32 >= FLOOR x max|ref|: an accidentally exact fp32 run gives no zero bound
EPS = 0.2
W = orc.LossWeights(lambda_policy=1.0, lambda_value=1.5, lambda_score=0.02, entropy_coeff=0.01, clip_epsilon=EPS)
GSCALE = 1024.0

# ------------------------------------------------------------------------------------------------ packed legal masks


def pack_mask_rows(legal: torch.Tensor) -> torch.Tensor:
    """(R, A) bool -> (R, ceil(A / 32)) int32: bit j of word w is action 32 w + j (csrc/rollout.hip, pack_mask_kernel)."""
    R, A = legal.shape
    words = (A + 31) // 32
    out = np.zeros((R, words), dtype=np.uint32)
    m = legal.numpy()
    for r in range(R):
        for a in np.flatnonzero(m[r]):
            out[r, a >> 5] |= np.uint32(1) << np.uint32(a & 31)
    return torch.from_numpy(out.view(np.int32))


def unpack_mask_rows(bits: torch.Tensor, A: int, mutant: Optional[str] = None) -> torch.Tensor:
    """(R, words) int32 -> (R, A) bool.  mutant "bit_order": bit j of a word read as action 32 w + 31 - j."""
    w = bits.numpy().view(np.uint32)
    R, words = w.shape
    out = np.zeros((R, words * 32), dtype=bool)
    for j in range(32):
        col = (31 - j) if mutant == "bit_order" else j
        out[:, col::32] = ((w >> np.uint32(j)) & np.uint32(1)).astype(bool)
    return torch.from_numpy(out[:, :A].copy())


# ------------------------------------------------------------------------------------------------ the bound


def e32_of(ref32: torch.Tensor, ref64: torch.Tensor) -> float:
    """max |fp32 run - fp64 run| of one reference formula over one tensor, floored at FLOOR x max|ref64|; infinities (the
    new_log_prob of an illegal action) must sit in the same places and are left out of both maxima."""
    fin = torch.isfinite(ref64)
    assert torch.equal(torch.isfinite(ref32), fin)
    if not bool(fin.any()):
        return 0.0
    r64 = ref64[fin].double()
    return max(float((ref32[fin].double() - r64).abs().max()), FLOOR * float(r64.abs().max()))


def excess(got: torch.Tensor, ref64: torch.Tensor, e32: float) -> float:
    """max |got - ref64| / e32 over the finite entries (inf where a non-finite entry differs, or the bound is 0 and got is
    not exact): a result passes when this is <= MARGIN."""
    fin = torch.isfinite(ref64)
    got = got.detach().cpu().reshape(ref64.shape)
    if not torch.equal(got[~fin].double(), ref64[~fin].double()):
        return math.inf
    err = float((got[fin].double() - ref64[fin].double()).abs().max()) if bool(fin.any()) else 0.0
    if not math.isfinite(err):                   # a NaN where the reference is finite
        return math.inf
    if err == 0.0:
        return 0.0
    return err / e32 if e32 > 0.0 else math.inf


def worst_excess(got: dict, ref: dict, e32: dict) -> Tuple[float, str]:
    """the largest excess() over the tensors that have a bound in `e32`, and its name"""
    return max((excess(got[k], ref[k], e32[k]), k) for k in e32)


# ------------------------------------------------------------------------------------------------ policy cases

POLICY_A = (1, 31, 32, 33, 255, 256, 257, 1023, 1024, 1025, 2049, 11259)
POLICY_SCALES = (3, 20)
PB, PS = 16, 24
SINGLE, ALL, LAST, ILLEGAL = 4, 6, 9, 15
# (target ratio, sign of the advantage) of logits row b; None = whatever the shared sample gives / no finite ratio
TABLE = ((0.5, 1), (0.79, 1), (0.5, -1), (0.79, -1), (0.81, 1), (1.0, -1), (1.19, 1), (0.81, -1), (1.19, -1), (1.21, -1),
         (1.5, -1), (1.21, 1), (1.5, 1), (1.0, 0), (None, 0), (None, 1))
TABLE_A1 = TABLE[:15] + ((1.5, 0),)              # A = 1 has no illegal action to choose
OUTCOMES = ("unclipped_below", "clipped_below", "in_range", "unclipped_above", "clipped_above")


class PolicyCase(NamedTuple):
    name: str
    A: int
    scale: int
    logits: torch.Tensor                         # (PB, A) float32
    legal: torch.Tensor                          # (PS, A) bool
    actions: torch.Tensor                        # (PS,) int64
    old_lp: torch.Tensor                         # (PS,) float32
    adv: torch.Tensor                            # (PS,) float32
    idx: torch.Tensor                            # (PB,) int64 into the PS samples, rows 13 and 14 equal


def _masked_lp64(logits, legal):
    return torch.log_softmax(logits.double().masked_fill(~legal, float("-inf")), dim=-1)


@functools.lru_cache(maxsize=None)
def policy_case(A: int, scale: int) -> PolicyCase:
    g = torch.Generator().manual_seed(100_000 * scale + A)
    table = TABLE_A1 if A == 1 else TABLE
    logits = (scale * torch.randn(PB, A, generator=g)).float()
    slots = torch.randperm(PS, generator=g)[:PB - 1]
    idx = slots[torch.tensor(list(range(14)) + [13, 14])].clone()
    legal = torch.rand(PS, A, generator=g) < 0.05
    actions = torch.randint(0, A, (PS,), generator=g)
    other = torch.randint(0, A, (PS,), generator=g)
    rows = torch.arange(PS)
    legal[rows, actions] = True
    legal[rows, other] = True
    if A > 1:
        s = int(idx[SINGLE]); legal[s] = False; legal[s, actions[s]] = True
        s = int(idx[ALL]); legal[s] = True; actions[s] = A - 1
        s = int(idx[LAST]); actions[s] = int(torch.randint(0, A - 1, (1,), generator=g)); legal[s] = False
        legal[s, actions[s]] = True; legal[s, A - 1] = True
        s = int(idx[ILLEGAL]); legal[s, actions[s]] = False; legal[s, (int(actions[s]) + 1) % A] = True
    old_lp = (-8.0 + 0.3 * torch.randn(PS, generator=g)).float()
    adv = torch.randn(PS, generator=g).float()
    mag = 0.5 + torch.rand(PB, generator=g)
    nlp = _masked_lp64(logits, legal[idx]).gather(1, actions[idx][:, None]).squeeze(1)
    for b in reversed(range(PB)):                # reversed: of two rows on one sample the FIRST one sets old_log_prob
        ratio, sign = table[b]
        s = int(idx[b])
        adv[s] = float(sign) * float(mag[b])
        if ratio is not None:
            old_lp[s] = float(nlp[b]) - math.log(ratio)
        elif not math.isfinite(float(nlp[b])):
            old_lp[s] = -5.0
    return PolicyCase(f"A{A}-s{scale}", A, scale, logits, legal, actions, old_lp, adv, idx)


POLICY_CASES = tuple((A, s) for s in POLICY_SCALES for A in POLICY_A)


def policy_ref(case: PolicyCase, dt: torch.dtype, mutant: Optional[str] = None, gscale: float = 1.0,
               legal: Optional[torch.Tensor] = None) -> dict:
    """new_lp, rowloss = -min(r adv, clamp(r, 1 - eps, 1 + eps) adv), rowent (entropy over the legal actions) per row and
    dlogits = d(gscale (w_policy sum rowloss - w_entropy sum rowent)) / dlogits by autograd, w_* = lambda / B, in `dt`.
    `legal`: the (PS, A) masks to use instead of the case's (the packed round trip).  Mutants: see MUTANTS_POLICY."""
    B = case.logits.shape[0]
    wp, we = W.lambda_policy / B, W.entropy_coeff / B
    idx = case.idx
    lg_all = case.logits.to(dt).clone().requires_grad_(True)
    lg = lg_all[idx % B] if mutant == "idx_on_logits" else lg_all
    legal = (case.legal if legal is None else legal)[idx]
    act, old, adv = case.actions[idx], case.old_lp[idx].to(dt), case.adv[idx].to(dt)
    ml = lg.masked_fill(~legal, float("-inf"))
    lp = torch.log_softmax(ml, dim=-1)
    if mutant == "no_onehot":
        new_lp = ml.gather(1, act[:, None]).squeeze(1).detach() - torch.logsumexp(ml, dim=-1)
    else:
        new_lp = lp.gather(1, act[:, None]).squeeze(1)
    if mutant == "entropy_all_actions":
        lpa = torch.log_softmax(lg, dim=-1)
        ent = -(lpa.exp() * lpa).sum(dim=-1)
    else:
        ent = -(lp.exp() * lp.masked_fill(~legal, 0.0)).sum(dim=-1)
    r = torch.exp(new_lp - old)
    rc = r.clamp(1 - EPS, 1 + EPS)
    if mutant == "clipped_gradient":
        rc = r + (rc - r).detach()
    rowloss = -torch.minimum(r * adv, rc * adv)
    ge = 1.0 if mutant == "entropy_unscaled" else gscale
    sign = 1.0 if mutant == "entropy_sign" else -1.0
    total = gscale * wp * rowloss.sum() + sign * ge * we * ent.sum()
    (dl,) = torch.autograd.grad(total, lg_all)
    return {"new_lp": new_lp.detach(), "rowloss": rowloss.detach(), "rowent": ent.detach(), "dlogits": dl}


# mutant -> does it show on the case?  (entropy_unscaled is judged on a run with the loss scale GSCALE)
MUTANTS_POLICY = {
    "entropy_all_actions": lambda c: c.A > 1,
    "entropy_sign": lambda c: c.A > 1,
    "clipped_gradient": lambda c: c.A > 1,       # (one action: its probability is 1 whatever the logit, all gradients 0)
    "idx_on_logits": lambda c: c.A > 1,
    "no_onehot": lambda c: True,
    "entropy_unscaled": lambda c: c.A > 1,
    "bit_order": lambda c: c.A > 1,
}


@functools.lru_cache(maxsize=None)
def policy_refs(A: int, scale: int, gscale: float = 1.0):
    """(float64 reference, e32 per tensor) of a policy case"""
    case = policy_case(A, scale)
    r64, r32 = policy_ref(case, torch.float64, gscale=gscale), policy_ref(case, torch.float32, gscale=gscale)
    return r64, {k: e32_of(r32[k], r64[k]) for k in r64}


def policy_conditions(case: PolicyCase) -> dict:
    """Asserts what the branch table promises, on the float64 reference, and returns the count per outcome: every realised
    ratio >= 0.005 from 1 +- eps (fp32 moves a ratio by ~1e-6: a correct kernel cannot land on the other branch), each of
    the five outcomes at least twice, the special rows what they claim to be."""
    ref = policy_ref(case, torch.float64)
    ratio = torch.exp(ref["new_lp"] - case.old_lp[case.idx].double())
    adv = case.adv[case.idx].double()
    table = TABLE_A1 if case.A == 1 else TABLE
    count = dict.fromkeys(OUTCOMES, 0)
    for b in range(PB):
        r, a = float(ratio[b]), float(adv[b])
        assert min(abs(r - (1 - EPS)), abs(r - (1 + EPS))) >= 0.005, (case.name, b, r)
        want, sign = table[b]
        assert (a > 0) - (a < 0) == sign, (case.name, b, a)
        if want is not None:
            assert abs(r - want) <= 1e-4 * want, (case.name, b, r, want)
        if a == 0.0 or r == 0.0:
            continue
        below, above = r < 1 - EPS, r > 1 + EPS
        key = ("unclipped_below" if a > 0 else "clipped_below") if below else \
              ("clipped_above" if a > 0 else "unclipped_above") if above else "in_range"
        count[key] += 1
    assert min(count.values()) >= 2, (case.name, count)
    assert int(case.idx[13]) == int(case.idx[14]) and case.idx.unique().numel() == PB - 1 and int(case.idx.max()) < PS
    if case.A > 1:
        legal = case.legal[case.idx]
        assert int(legal[SINGLE].sum()) == 1 and float(ref["rowent"][SINGLE]) == 0.0
        assert bool((ref["dlogits"][SINGLE] == 0).all())
        assert bool(legal[ALL].all()) and int(case.actions[case.idx[ALL]]) == case.A - 1
        assert legal[LAST].nonzero().flatten().tolist() == sorted({int(case.actions[case.idx[LAST]]), case.A - 1})
        assert not bool(legal[ILLEGAL, case.actions[case.idx[ILLEGAL]]]) and bool(legal[ILLEGAL].any())
        assert float(ref["new_lp"][ILLEGAL]) == -math.inf and float(ratio[ILLEGAL]) == 0.0
        assert bool(torch.isfinite(ref["dlogits"]).all()) and float(ref["rowloss"][ILLEGAL]) == 0.0
        assert bool((ref["dlogits"][~legal] == 0).all())
    return count


# ------------------------------------------------------------------------------------------------ value cases

VALUE_B = (1, 63, 64, 65, 1023, 1024, 1025, 2049, 5000)
VALUE_CASES = tuple((B, "mixed") for B in VALUE_B) + ((1025, "ignored"), (1025, "valid"))
TIE_ROWS = ((0.75, 0.75, -0.5), (-1.25, 0.5, 0.5), (0.25, 0.25, 0.25))      # argmax 0, 1, 0: the first maximum
TIE_PRED = (0, 1, 0)
MIN_GAP = 1e-3


class ValueCase(NamedTuple):
    name: str
    kind: str
    B: int
    vlogits: torch.Tensor                        # (B, 3) float32
    score: torch.Tensor                          # (B,)
    cats: torch.Tensor                           # (S,) int64 in {-1, 0, 1, 2}, S = B + 7
    targets: torch.Tensor                        # (S,)
    idx: torch.Tensor                            # (B,) into S, with repeats
    rowloss: torch.Tensor                        # (B,) the policy kernel's outputs, here just data
    rowent: torch.Tensor                         # (B,)


@functools.lru_cache(maxsize=None)
def value_case(B: int, kind: str = "mixed", salt: int = 0) -> ValueCase:
    g = torch.Generator().manual_seed(7919 * B + 31 * salt + {"mixed": 0, "ignored": 1, "valid": 2}[kind])
    S = B + 7
    vl = (2.0 * torch.randn(B, 3, generator=g)).float()
    top = vl.topk(2, dim=1).values
    vl[(top[:, 0] - top[:, 1]) < 10 * MIN_GAP, 0] += 0.5
    nt = min(B, 3)
    vl[:nt] = torch.tensor(TIE_ROWS)[:nt]
    idx = torch.randperm(S, generator=g)[:B]
    if B > 3:                                    # ~10 % of the rows fetch a sample another row fetches too
        rep = 3 + torch.randperm(B - 3, generator=g)[:max(1, B // 10)]
        idx[rep] = idx[torch.randint(0, B, (rep.numel(),), generator=g)]
    cats = torch.randint(0, 3, (S,), generator=g)
    if kind == "mixed":
        cats[torch.rand(S, generator=g) < 0.3] = -1
        cats[idx[:nt]] = torch.tensor([0, 2, 1])[:nt]        # the tie rows count: one predicted right, two wrong
    elif kind == "ignored":
        cats[:] = -1
    return ValueCase(f"B{B}-{kind}" + (f"-{salt}" if salt else ""), kind, B, vl, torch.randn(B, generator=g).float(), cats,
                     torch.randn(S, generator=g).clamp(-1.5, 1.5).float(), idx, torch.randn(B, generator=g).float(),
                     (1.0 + torch.rand(B, generator=g)).float())


def value_conditions(case: ValueCase) -> None:
    """the designated tie rows are exact ties, every other row's top two logits are >= MIN_GAP apart, idx has repeats"""
    nt = min(case.B, 3)
    assert torch.equal(case.vlogits[:nt], torch.tensor(TIE_ROWS)[:nt])
    if case.B > nt:
        top = case.vlogits[nt:].double().topk(2, dim=1).values
        assert float((top[:, 0] - top[:, 1]).min()) >= MIN_GAP, case.name
    assert int(case.idx.max()) < case.B + 7
    if case.B > 3:
        assert case.idx.unique().numel() < case.B
    valid = case.cats[case.idx] >= 0
    if case.kind == "ignored":
        assert not bool(valid.any())
    elif case.kind == "valid":
        assert bool(valid.all())
    else:
        assert bool(valid[:nt].all())
        if case.B >= 63:
            assert 0.15 < 1.0 - float(valid.float().mean()) < 0.45, case.name


def value_ref(case: ValueCase, dt: torch.dtype, combined: int, mutant: Optional[str] = None, gscale: float = 1.0,
              use_idx: bool = True) -> dict:
    """out[0..4] = policy loss, value CE (ignore_index -1, mean over the VALID rows, 0 when there is none), score MSE over
    B, entropy, total; counts = (n_valid, predicted right, predicted win, predicted draw) as integers, the argmax being
    the FIRST maximum; dvlogits / dscore = d(gscale (lambda_v ce + lambda_s mse)); acc = what one call adds to the four
    running sums (combined_value_metric: the value slot takes lambda_v ce + lambda_s mse and the score slot 0).
    use_idx=False: row b's sample is b (the identity the kernel takes for a null index)."""
    B = case.B
    idx = case.idx if use_idx else torch.arange(B)
    vl = case.vlogits.to(dt).clone().requires_grad_(True)
    sc = case.score.to(dt).clone().requires_grad_(True)
    cats, tg = case.cats[idx], case.targets[idx].to(dt)
    valid = cats >= 0
    n_valid = int(valid.sum())
    lp = torch.log_softmax(vl, dim=-1)
    rows = -lp.gather(1, cats.clamp(min=0)[:, None]).squeeze(1)
    den = B if mutant == "ce_over_B" else n_valid
    ce = (rows * valid.to(dt)).sum() / den if n_valid > 0 else vl.sum() * 0.0
    mse = ((sc - tg) ** 2).mean()
    vs = W.lambda_value * ce + W.lambda_score * mse
    dv, ds = torch.autograd.grad(gscale * vs, [vl, sc])
    if mutant == "score_no_2":
        ds = ds * 0.5
    pl, ent = case.rowloss.to(dt).mean(), case.rowent.to(dt).mean()
    total = W.lambda_policy * pl + vs - W.entropy_coeff * ent
    v = case.vlogits
    if mutant == "tie_last":
        pred = 2 - v.flip(1).argmax(dim=1)
    else:
        pred = torch.where((v[:, 0] >= v[:, 1]) & (v[:, 0] >= v[:, 2]), 0, torch.where(v[:, 1] >= v[:, 2], 1, 2))
    counts = (n_valid, int((pred == cats)[valid].sum()), int((pred == 0)[valid].sum()), int((pred == 1)[valid].sum()))
    zero = torch.zeros((), dtype=dt)
    acc = torch.stack([pl, vs if combined else ce, zero if combined else mse, ent]).detach()
    return {"out": torch.stack([pl, ce, mse, ent, total]).detach(), "dvlogits": dv, "dscore": ds, "acc": acc,
            "counts": counts}


def value_fractions(counts) -> list:
    """out[5..8] as the kernel must store them: n_valid, then count / n_valid divided in double and rounded once"""
    n = counts[0]
    return [float(n)] + [float(np.float32(c / n)) if n > 0 else 0.0 for c in counts[1:]]


MUTANTS_VALUE = {
    "ce_over_B": lambda c, use_idx=True: 0 < int((c.cats[c.idx if use_idx else torch.arange(c.B)] >= 0).sum()) < c.B,
    "score_no_2": lambda c, use_idx=True: True,
    "tie_last": lambda c, use_idx=True: bool((c.cats[c.idx if use_idx else torch.arange(c.B)] >= 0)[:3].any()),
}
VALUE_TENSORS = ("out", "dvlogits", "dscore", "acc")


@functools.lru_cache(maxsize=None)
def value_refs(B: int, kind: str, combined: int, use_idx: bool = True, gscale: float = 1.0, salt: int = 0):
    case = value_case(B, kind, salt)
    r64 = value_ref(case, torch.float64, combined, gscale=gscale, use_idx=use_idx)
    r32 = value_ref(case, torch.float32, combined, gscale=gscale, use_idx=use_idx)
    return r64, {k: e32_of(r32[k], r64[k]) for k in VALUE_TENSORS}


# ------------------------------------------------------------------------------------------------ the small kernels


def policy_ce_ref(case: PolicyCase, dt: torch.dtype) -> dict:
    """ka_policy_ce: rowloss = logsumexp(row) - row[target], dlogits = w (softmax - onehot), w = lambda_policy / B; the
    targets are the case's per-sample actions, fetched through idx."""
    lg = case.logits.to(dt).clone().requires_grad_(True)
    rows = -torch.log_softmax(lg, dim=-1).gather(1, case.actions[case.idx][:, None]).squeeze(1)
    (dl,) = torch.autograd.grad(W.lambda_policy / lg.shape[0] * rows.sum(), lg)
    return {"rowloss": rows.detach(), "dlogits": dl}


def masked_softmax_ref(case: PolicyCase, dt: torch.dtype) -> dict:
    legal = case.legal[case.idx]
    return {"probs": torch.softmax(case.logits.to(dt).masked_fill(~legal, float("-inf")), dim=-1)}


def scalar_value_ref(case: ValueCase, alpha: float, dt: torch.dtype) -> dict:
    return {"value": orc.scalar_value_blended(case.vlogits.to(dt), (3.0 * case.score).to(dt)[:, None], alpha)}


NORMALIZE_N = (2, 3, 1023, 1024, 1025, 65537)


@functools.lru_cache(maxsize=None)
def normalize_case(n: int) -> torch.Tensor:
    return (3.0 + torch.randn(n, generator=torch.Generator().manual_seed(n))).float()


def normalize_ref(x: torch.Tensor, dt: torch.dtype) -> dict:
    return {"out": orc.normalize_advantages(x.to(dt))}


def with_e32(fn, *args):
    """(float64 reference, e32 per tensor) of fn(*args, dtype)"""
    r64, r32 = fn(*args, torch.float64), fn(*args, torch.float32)
    return r64, {k: e32_of(r32[k], r64[k]) for k in r64}


GAE_SHAPES = ((1, 1), (1, 65), (7, 63), (128, 64))


def gae_case(T: int, N: int, f64: bool):
    """rewards, values, terminated, next_value, override (NaN = none), lengths with a 0 (and a T where N > 1)"""
    rng = np.random.default_rng(1000 * T + N)
    dt = np.float64 if f64 else np.float32
    r, v = rng.standard_normal((T, N)).astype(dt), rng.standard_normal((T, N)).astype(dt)
    term = (rng.random((T, N)) < 0.1).astype(np.float32)
    nv = rng.standard_normal(N).astype(dt)
    ov = np.where(rng.random((T, N)) < 0.2, rng.standard_normal((T, N)), np.nan).astype(dt)
    lengths = rng.integers(0, T + 1, N).astype(np.int64)
    lengths[0] = 0
    if N > 1:
        lengths[-1] = T
    return r, v, term, nv, ov, lengths


# ------------------------------------------------------------------------------------------------ optimiser

ADAM_SIZES = (1, 255, 256, 257, 4095, 4096, 4097, 8191, 12289)
ADAM_TAIL = tuple(n % 256 != 0 for n in ADAM_SIZES)
ADAM_GRAD_SCALES = (4.0, 0.002, 0.4)             # global norms ~12, ~0.006, ~1.2: clipped hard, not clipped, in between
ADAM_LR, ADAM_MAX_NORM = 2e-4, 1.0
# The C ABI carries the betas as fp32, so the reference is given the betas the kernel receives: 0.9f and 0.999f.  It
# matters for beta2 only: 1 - 0.999f is 1.3e-5 below 1 - 0.999, a factor exp_avg_sq carries (and the bias correction
# 1 - beta2^t with it, so the update agrees either way); held to beta2 = 0.999 itself, exp_avg_sq would sit outside
# the moments' rtol of 1e-5 wherever it exceeds ~3e-5 (the one-element tensor here).
ADAM_BETAS = (float(np.float32(0.9)), float(np.float32(0.999)))


@functools.lru_cache(maxsize=None)
def adam_case():
    """(initial parameters, gradients of the three steps) over the odd-sized table"""
    g = torch.Generator().manual_seed(77)
    params = tuple(torch.randn(n, generator=g) for n in ADAM_SIZES)
    grads = tuple(tuple(s * torch.randn(n, generator=g) / n ** 0.5 for n in ADAM_SIZES) for s in ADAM_GRAD_SCALES)
    return params, grads


def adam_ref(mutant: Optional[str] = None, dt: torch.dtype = torch.float32) -> dict:
    """Three steps of orc.clip_and_adam: the parameters after each step, the final moments, the three norms and clip
    coefficients.  mutant "tail_dropped": the elements past the last full 256 of a tensor are left as they were."""
    p0, grads = adam_case()
    p = [t.clone().to(dt) for t in p0]
    m, v = [torch.zeros_like(t) for t in p], [torch.zeros_like(t) for t in p]
    out = {"params": [], "norms": [], "coefs": []}
    for s in range(3):
        keep = [[t.clone() for t in (a, b, c)] for a, b, c in zip(p, m, v)]
        norm = orc.clip_and_adam(p, [t.clone().to(dt) for t in grads[s]], m, v, s + 1, ADAM_LR, ADAM_MAX_NORM,
                                 beta1=ADAM_BETAS[0], beta2=ADAM_BETAS[1])
        if mutant == "tail_dropped":
            for i, old in enumerate(keep):
                cut = ADAM_SIZES[i] & ~255
                for new, o in zip((p[i], m[i], v[i]), old):
                    new[cut:] = o[cut:]
        out["params"].append([t.clone() for t in p])
        out["norms"].append(float(norm))
        out["coefs"].append(min(1.0, ADAM_MAX_NORM / (float(norm) + 1e-6)))
    out["m"], out["v"] = m, v
    return out


def adam_mismatch(got: dict, ref: dict) -> list:
    """indices of the tensors of `got` outside the optimiser bounds against `ref` (parameters 2e-6 after each step, moments
    rtol 1e-5 / atol 1e-8 and 1e-10) -- the class of the golden and the full-size test"""
    bad = set()
    for s in range(3):
        for i, (a, b) in enumerate(zip(got["params"][s], ref["params"][s])):
            if float((a.double() - b.double()).abs().max()) > 2e-6:
                bad.add(i)
    for i in range(len(ADAM_SIZES)):
        if not torch.allclose(got["m"][i].float(), ref["m"][i].float(), rtol=1e-5, atol=1e-8):
            bad.add(i)
        if not torch.allclose(got["v"][i].float(), ref["v"][i].float(), rtol=1e-5, atol=1e-10):
            bad.add(i)
    return sorted(bad)


def scaler_rule(scale: float, tracker: float, finite: bool, growth: float = 2.0, backoff: float = 0.5, interval: int = 2000):
    """torch.amp.GradScaler.update() from its documented semantics: a non-finite gradient norm multiplies the scale by
    backoff_factor and clears the growth tracker; otherwise the tracker counts one more clean step and, on reaching
    growth_interval, the scale is multiplied by growth_factor and the tracker cleared.  Returns (scale, tracker)."""
    if not finite:
        return scale * backoff, 0.0
    tracker += 1.0
    if tracker >= interval:
        return scale * growth, 0.0
    return scale, tracker
