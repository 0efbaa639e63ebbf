"""ka_policy_sample_ctl (csrc/sampling.hip) on the device: the neutral row against the play sampler bit for bit, greedy and
top-1, the distributions under temperature and cut against the float64 restatement, per-model rows with the opening switch,
the table re-read and the flags."""
import math
import struct

import numpy as np
import pytest
import torch

from keisei_amd import _lib
from keisei_amd.training import SamplingControls, controls_table, sample_controlled

pytestmark = pytest.mark.gpu
DEV = "cuda"
BIG = 9 * 9 * 139
GREEDY, NEUTRAL = SamplingControls.GREEDY, SamplingControls.NEUTRAL


def _stream():
    return _lib.stream_ptr(torch.device(DEV))


def _out(B):
    return (torch.empty(B, dtype=torch.int64, device=DEV), torch.empty(B, device=DEV),
            torch.empty(B, dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV))


def _play(logits, legal, words, seed_dev, model_of, K):
    B, A = logits.shape
    out = _out(B)
    _lib.call("ka_policy_sample_play", logits, int(logits.dtype == torch.bfloat16), legal, words, seed_dev, model_of, K,
              *out, B, A, _stream())
    return out


def _ctl(logits, legal, words, seed_dev, model_of, table, plies=None, stride=0):
    B, A = logits.shape
    out = _out(B)
    _lib.call("ka_policy_sample_ctl", logits, int(logits.dtype == torch.bfloat16), legal, words, seed_dev, model_of,
              table.shape[0], table, plies, stride, *out, B, A, _stream())
    return out


def _table(sampling, K):
    return torch.from_numpy(controls_table(sampling, K)).to(DEV)


def _pack(masks):
    B, A = masks.shape
    bits = torch.zeros(B, (A + 31) // 32, dtype=torch.int32, device=DEV)
    _lib.call("ka_pack_mask_bits", masks.to(DEV).contiguous(), bits, B, A, _stream())
    return bits


def _rows(B, A, seed, density):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, A, generator=g) * 2
    masks = torch.rand(B, A, generator=g) < density
    masks[0] = False
    masks[0, A - 7] = True                                   # a single legal action
    masks[1] = True                                          # everything legal
    masks[:, 5] |= ~masks.any(dim=1)
    return logits, masks


def _seed(v):
    return torch.tensor([v], dtype=torch.int64, device=DEV)


# ------------------------------------------------------------------ the neutral row
@pytest.mark.parametrize("A,packed", [(53, False), (BIG, True)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_neutral_row_is_the_play_sampler_bit_for_bit(A, packed, dtype):
    B, K = 7, 2
    logits, masks = _rows(B, A, 11, 0.5 if A == 53 else 0.03)
    logits = logits.to(DEV).to(dtype)
    legal, words = (_pack(masks), (A + 31) // 32) if packed else (masks.to(DEV), 0)
    model_of = torch.tensor([0, 1, 0, -1, 1, 0, 1], dtype=torch.int32, device=DEV)           # row 3 is unseated
    plies = torch.arange(B, dtype=torch.int32, device=DEV)
    # neutral in effect: T == 1 and no cut on either side of an opening
    tables = [_table(None, K), _table(SamplingControls(1.0, 1.0, 3, 0), K)]
    for seed in (0, 0x1234_5678_9ABC_DEF0 - (1 << 62), -5):
        want = _play(logits, legal, words, _seed(seed), model_of, K)
        for table in tables:
            for pl, stride in ((None, 0), (plies, 4)):
                got = _ctl(logits, legal, words, _seed(seed), model_of, table, pl, stride)
                for name, w, g in zip(("actions", "logp", "nlegal", "flags"), want, got):
                    assert torch.equal(w, g), (name, seed)
    assert int(want[0][0]) == A - 7 and int(want[2][1]) == A
    assert int(want[0][3]) == int(masks[3].int().argmax()) and float(want[1][3]) == 0.0


# ------------------------------------------------------------------ greedy and top-1
@pytest.mark.parametrize("A,packed", [(53, False), (BIG, True)])
def test_greedy_and_top1_are_the_host_argmax(A, packed):
    B = 7
    logits, masks = _rows(B, A, 12, 0.5 if A == 53 else 0.03)
    for b, (i, j, bad) in {2: (9, 40, 20), 4: (A - 3, A - 30, 1), 5: (0, A - 1, 30)}.items():
        masks[b, [i, j]] = True                              # the maximum twice at legal indices, once at an illegal one
        masks[b, bad] = False
        logits[b, [i, j, bad]] = 40.0
    want = logits.masked_fill(~masks, float("-inf")).argmax(dim=1)
    for b, first in ((2, 9), (4, A - 30), (5, 0)):
        want[b] = first
    host = sample_controlled(logits, masks, 1, controls=GREEDY)
    assert torch.equal(host.actions, want)
    legal, words = (_pack(masks), (A + 31) // 32) if packed else (masks.to(DEV), 0)
    model_of = torch.zeros(B, dtype=torch.int32, device=DEV)
    for c in (GREEDY, SamplingControls(1.0, top_k=1), SamplingControls(0.5, top_k=1), SamplingControls(0.0, top_k=7)):
        for seed in (3, 4):
            act, lp, nl, flags = _ctl(logits.to(DEV), legal, words, _seed(seed), model_of, _table(c, 1))
            assert torch.equal(act.cpu(), want), c
            assert float(lp.abs().max()) <= 2e-7, c
            assert torch.equal(nl.cpu(), masks.sum(1).int()) and flags.tolist() == [0, 0]


# ------------------------------------------------------------------ the distributions
DIST_SEED = 3


def _dist_rows():
    g = torch.Generator().manual_seed(DIST_SEED)
    B, A = 6, 53
    logits = torch.randn(B, A, generator=g) * 2
    masks = torch.rand(B, A, generator=g) < 0.6
    masks[0] = False
    masks[0, 17] = True                                      # a single legal action
    masks[1] = True                                          # everything legal
    masks[:, 5] |= ~masks.any(dim=1)
    return logits, masks


@pytest.mark.parametrize("T,k", [(0.5, 0), (2.0, 0), (0.5, 5), (1.0, 5)])
def test_draws_follow_the_host_distribution(T, k):
    """40 000 draws per row: 50 repeats of the rows per launch (the uniform depends on (seed, row)), 800 seeds.  The float64
    restatement alone, drawing with the same uniforms, passes the frequency bound for this generator seed (run on the host
    when the test was written: its worst deviation over the four controls is 3.81 sigma, against the bound of 4.5), and fp32
    log_softmax(z / T) in torch stays inside the log-prob tolerance for these logits at all four controls, T = 0.5 included."""
    logits, masks = _dist_rows()
    B, A = logits.shape
    c = SamplingControls(T, top_k=k)
    host = sample_controlled(logits, masks, 0, controls=c)
    p = host.probs.to(DEV)                                   # (B, A) float64: the distribution, whatever the seed
    eps = 1.1920928955078125e-07
    ref_lp = p.clamp(eps, 1 - eps).log().float()             # Categorical.log_prob's clamp, in float64
    draws, reps = 40000, 50
    big, bigm = logits.repeat(reps, 1).to(DEV), masks.repeat(reps, 1).to(DEV)
    table, model_of = _table(c, 1), torch.zeros(B * reps, dtype=torch.int32, device=DEV)
    rows = torch.arange(B, device=DEV).repeat(reps)
    counts = torch.zeros(B, A, device=DEV)
    outside = torch.zeros((), dtype=torch.int64, device=DEV)
    lp_err = torch.zeros((), device=DEV)
    seed_dev = _seed(0)
    for _ in range(draws // reps):
        act, lp, nl, flags = _ctl(big, bigm, 0, seed_dev, model_of, table)
        seed_dev.add_(1)
        outside += (p[rows, act] <= 0).sum()
        want = ref_lp[rows, act]
        lp_err = torch.maximum(lp_err, ((lp - want).abs() - 1e-5 * want.abs()).max())
        counts.index_put_((rows, act), torch.ones(B * reps, device=DEV), accumulate=True)
    assert flags.tolist() == [0, 0] and torch.equal(nl[:B].cpu(), masks.sum(1).int())
    assert int(outside) == 0                                 # every draw lies in the host support
    assert float(lp_err) <= 1e-5
    sigma = (p * (1 - p) / draws).sqrt()
    dev = (counts.double() / draws - p).abs()
    assert bool((dev <= 4.5 * sigma + 1e-4).all()), float((dev / (sigma + 1e-9)).max())
    assert counts[0, 17] == draws
    if k:
        assert int((counts > 0).sum(dim=1).max()) <= k


# ------------------------------------------------------------------ per-model rows and the opening switch
def test_per_model_rows_and_the_opening_switch_in_one_launch():
    A, K, stride = BIG, 3, 128
    ctl = [SamplingControls(0.5, 2.0, 4, 6), SamplingControls(0.0, 1.0, 9, 0), SamplingControls(1.5, 0.0, 2, 3)]
    opening = [c.opening_plies for c in ctl]
    model_of, plies = [], []
    for m in range(K):
        for d in (-1, 0, 1):
            model_of.append(m)
            plies.append(opening[m] + d)
    model_of += [-1, K, 0, 1]
    plies += [0, 3, 0xFFFFFFFF, 0]
    B = len(model_of)
    g = torch.Generator().manual_seed(21)
    logits = (torch.randn(B, A, generator=g) * 2).to(DEV)
    masks = torch.rand(B, A, generator=g) < 0.01
    masks[:, 0] = False
    masks[:, 77] = True
    bits = _pack(masks)
    state = torch.zeros(B, stride, dtype=torch.uint8)        # a fake env state: the game ply is the u32 at byte 100
    state[:, 100:104] = torch.from_numpy(np.array(plies, dtype=np.uint32).view(np.uint8).reshape(B, 4))
    state[:, 96:100] = 0xEE
    state[:, 104:108] = 0xEE
    state = state.to(DEV)
    mo = torch.tensor(model_of, dtype=torch.int32, device=DEV)
    seed = _seed(99)
    table = _table(ctl, K)
    act, lp, nl, flags = _ctl(logits, bits, bits.shape[1], seed, mo, table, state.data_ptr() + 100, stride)
    assert flags.tolist() == [0, 0] and torch.equal(nl.cpu(), masks.sum(1).int())
    effective = {}
    for b in range(B):
        m = model_of[b]
        if 0 <= m < K:
            effective.setdefault(ctl[m].effective(plies[b]), []).append(b)
    assert len(effective) == 6
    for c, rows in effective.items():                        # a launch whose table holds that single control for all models
        a1, l1, _, _ = _ctl(logits, bits, bits.shape[1], seed, mo, _table(c, K), state.data_ptr() + 100, stride)
        a2, l2, _, _ = _ctl(logits, bits, bits.shape[1], seed, mo, _table(c, K))                # no plies: opening_plies = 0
        assert torch.equal(a1, a2) and torch.equal(l1, l2)
        assert torch.equal(act[rows], a1[rows]) and torch.equal(lp[rows], l1[rows]), c
    unseated = [b for b in range(B) if not 0 <= model_of[b] < K]
    first = masks.int().argmax(dim=1)
    assert len(unseated) == 2
    assert torch.equal(act[unseated].cpu(), first[unseated]) and bool((lp[unseated] == 0).all())
    # the greedy rows of model 1 (behind its opening) and of model 2 (inside it) are the arg-max
    best = logits.cpu().masked_fill(~masks, float("-inf")).argmax(dim=1)
    for b in (4, 5, 6):
        assert int(act[b]) == int(best[b]) and abs(float(lp[b])) <= 2e-7, b
    # the whole launch is the host restatement's (the draws are far from a rounding boundary at these sizes)
    host = sample_controlled(logits.cpu(), masks, 99, controls=ctl, model_of=mo.cpu(), plies=torch.tensor(plies))
    assert torch.equal(host.actions, act.cpu())
    assert torch.allclose(host.log_probs.float(), lp.cpu(), atol=1e-5, rtol=1e-5)
    assert torch.equal(sample_controlled(logits, bits, 99, controls=ctl, model_of=mo, plies=torch.tensor(plies)).actions, act)


# ------------------------------------------------------------------ the table is read on every launch
def test_table_is_read_again_on_every_launch():
    B, A = 16, BIG
    g = torch.Generator().manual_seed(5)
    logits = (torch.randn(B, A, generator=g) * 2).to(DEV)
    masks = torch.rand(B, A, generator=g) < 0.02
    bits = _pack(masks)
    mo = torch.zeros(B, dtype=torch.int32, device=DEV)
    seed = _seed(31)
    table = _table(None, 1)
    ptr = table.data_ptr()
    first = _ctl(logits, bits, bits.shape[1], seed, mo, table)
    assert torch.equal(first[0], _play(logits, bits, bits.shape[1], seed, mo, 1)[0])
    table.copy_(torch.from_numpy(controls_table(GREEDY, 1)))
    assert table.data_ptr() == ptr
    second = _ctl(logits, bits, bits.shape[1], seed, mo, table)
    best = logits.masked_fill(~masks.to(DEV), float("-inf")).argmax(dim=1)
    assert torch.equal(second[0], best) and not torch.equal(first[0], second[0])
    # a row the Python layer would refuse is read as the neutral row
    table.copy_(torch.from_numpy(np.frombuffer(struct.pack("<ffii", 0.5, 0.5, 0, 65), dtype=np.int32).reshape(1, 4).copy()))
    third = _ctl(logits, bits, bits.shape[1], seed, mo, table)
    assert torch.equal(third[0], first[0]) and torch.equal(third[1], first[1])


# ------------------------------------------------------------------ flags and refusals
@pytest.mark.parametrize("c", [NEUTRAL, GREEDY, SamplingControls(0.5, top_k=4)], ids=["neutral", "greedy", "cut"])
def test_flags(c):
    B, A = 5, 53
    logits, masks = _rows(B, A, 13, 0.5)
    masks[3] = False
    mo = torch.zeros(B, dtype=torch.int32, device=DEV)
    act, lp, nl, flags = _ctl(logits.to(DEV), masks.to(DEV), 0, _seed(1), mo, _table(c, 1))
    assert flags.tolist() == [0, 1] and int(act[3]) == 0 and float(lp[3]) == 0.0 and int(nl[3]) == 0
    logits[2, 9] = float("nan")
    masks[3, 4] = True
    flags = _ctl(logits.to(DEV), masks.to(DEV), 0, _seed(1), mo, _table(c, 1))[3]
    assert flags.tolist() == [1, 0]


def test_entry_point_refusals():
    B, A = 4, 53
    logits, masks = _rows(B, A, 14, 0.5)
    logits, masks = logits.to(DEV), masks.to(DEV)
    mo = torch.zeros(B, dtype=torch.int32, device=DEV)
    table, seed, out = _table(None, 1), _seed(1), _out(B)
    plies = torch.zeros(B, dtype=torch.int32, device=DEV)

    def call(**kw):
        a = dict(logits=logits, legal=masks, words=0, seed=seed, mo=mo, K=1, table=table, plies=None, stride=0, A=A)
        a.update(kw)
        _lib.call("ka_policy_sample_ctl", a["logits"], 0, a["legal"], a["words"], a["seed"], a["mo"], a["K"], a["table"],
                  a["plies"], a["stride"], *out, B, a["A"], _stream())

    call()
    for kw, msg in (({"table": None}, "null tensor"), ({"seed": None}, "null tensor"), ({"words": 3}, "packed mask rows"),
                    ({"K": 0}, "at least one row"), ({"plies": plies, "stride": 0}, "ply_stride"),
                    ({"A": 20000}, "too large for the LDS row")):
        with pytest.raises(_lib.KeiseiHipError, match=msg):
            call(**kw)
    assert math.isfinite(float(out[1].sum()))
