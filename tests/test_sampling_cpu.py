"""Sampling controls (keisei_amd/training/sampling.py): the controls table, the float64 restatement of
ka_policy_sample_ctl and the owners' argument checks -- everything that runs without a GPU."""
import ctypes
import math
import struct

import numpy as np
import pytest
import torch

from keisei_amd import _lib
from keisei_amd.training import ControlledSample, SamplingControls, controls_table, sample_controlled
from keisei_amd.training.sampling import arena_controls, league_controls, sample_uniform

EPS = 1.1920928955078125e-07
GREEDY, NEUTRAL = SamplingControls.GREEDY, SamplingControls.NEUTRAL


def test_entry_point_is_exported():
    lib = ctypes.CDLL(str(_lib.library_path()))
    assert hasattr(lib, "ka_policy_sample_ctl")
    assert "ka_policy_sample_ctl" in _lib.exported_symbols()
    assert len(_lib._SIGS["ka_policy_sample_ctl"].replace(" ", "")) == 17


# ------------------------------------------------------------------ controls
def test_controls_defaults_and_constants():
    c = SamplingControls()
    assert (c.temperature, c.opening_temperature, c.opening_plies, c.top_k) == (1.0, None, 0, 0)
    assert NEUTRAL == c and GREEDY == SamplingControls(temperature=0.0)
    with pytest.raises(Exception):                          # frozen
        c.temperature = 2.0


@pytest.mark.parametrize("kw", [
    {"temperature": -0.1}, {"temperature": float("nan")}, {"temperature": float("inf")}, {"temperature": "1"},
    {"opening_temperature": -1.0}, {"opening_temperature": float("inf")}, {"opening_temperature": float("nan")},
    {"opening_plies": -1}, {"opening_plies": 65536}, {"opening_plies": 1.5}, {"opening_plies": True},
    {"top_k": -1}, {"top_k": 65}, {"top_k": 2.0}, {"top_k": True},
])
def test_controls_refusals(kw):
    with pytest.raises(ValueError):
        SamplingControls(**kw)


def test_controls_accept_the_edges():
    SamplingControls(temperature=0, opening_temperature=0.0, opening_plies=65535, top_k=64)
    SamplingControls(temperature=3, top_k=1)


def test_table_layout_is_bit_cast():
    t = controls_table([SamplingControls(0.5, 2.0, 6, 5), SamplingControls(0.25, top_k=3)], 2)
    assert t.dtype == np.int32 and t.shape == (2, 4)
    assert t[0].tobytes() == struct.pack("<ffii", 0.5, 2.0, 6, 5)
    assert t[1].tobytes() == struct.pack("<ffii", 0.25, 0.25, 0, 3)          # opening_temperature=None means temperature
    assert t[0].view(np.float32)[0] == 0.5 and t[0, 2] == 6 and t[0, 3] == 5
    n = controls_table(None, 3)
    assert n.shape == (3, 4) and all(r.tobytes() == struct.pack("<ffii", 1.0, 1.0, 0, 0) for r in n)
    assert np.array_equal(controls_table(GREEDY, 2), np.stack([GREEDY.row()] * 2))


def test_table_refusals():
    with pytest.raises(ValueError, match="expected 3"):
        controls_table([NEUTRAL, GREEDY], 3)
    with pytest.raises(ValueError, match="SamplingControls"):
        controls_table([NEUTRAL, 0.5], 2)
    with pytest.raises(ValueError, match="sampling must be"):
        controls_table(0.5, 2)
    with pytest.raises(ValueError, match="at least one row"):
        controls_table(None, 0)


# ------------------------------------------------------------------ owners' validation
def test_arena_argument_checks():
    assert arena_controls(None, 2, collect=False) is None and arena_controls(None, 2, collect=True) is None
    with pytest.raises(ValueError, match="collect=True"):
        arena_controls(GREEDY, 2, collect=True)
    with pytest.raises(ValueError, match="collect=True"):
        arena_controls([NEUTRAL, NEUTRAL], 2, collect=True)               # even neutral rows: the graph holds the other sampler
    with pytest.raises(ValueError, match="expected 2"):
        arena_controls([GREEDY], 2, collect=False)
    assert np.array_equal(arena_controls(GREEDY, 2, collect=False), controls_table(GREEDY, 2))


def test_league_argument_checks():
    assert league_controls(None, 3) is None
    t = league_controls(GREEDY, 3)
    assert t.shape == (4, 4) and np.array_equal(t[0], NEUTRAL.row()) and np.array_equal(t[1:], controls_table(GREEDY, 3))
    per = [GREEDY, SamplingControls(2.0), SamplingControls(0.5, top_k=4)]
    t = league_controls(per, 3)
    assert np.array_equal(t[0], NEUTRAL.row()) and np.array_equal(t[1:], controls_table(per, 3))
    with pytest.raises(ValueError, match="one per opponent"):
        league_controls(per, 2)
    with pytest.raises(ValueError):
        league_controls(0.5, 2)


# ------------------------------------------------------------------ the host restatement
def _rows(B=5, A=53, seed=1):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, A, generator=g) * 2
    masks = torch.rand(B, A, generator=g) < 0.6
    masks[:, 5] = True
    return logits, masks


def _pack(masks):
    B, A = masks.shape
    W = (A + 31) // 32
    padded = np.zeros((B, W * 32), np.uint32)
    padded[:, :A] = masks.numpy()
    words = (padded.reshape(B, W, 32) << np.arange(32, dtype=np.uint32)).sum(axis=2, dtype=np.uint64).astype(np.uint32)
    return torch.from_numpy(words.view(np.int32))


def test_neutral_probs_are_the_masked_softmax():
    logits, masks = _rows()
    r = sample_controlled(logits, masks, 9, controls=None)
    assert isinstance(r, ControlledSample)
    ref = torch.softmax(logits.double().masked_fill(~masks, float("-inf")), dim=-1)
    assert torch.allclose(r.probs, ref, atol=1e-15, rtol=1e-13)
    rows = torch.arange(len(logits))
    assert bool(masks[rows, r.actions].all())
    assert torch.allclose(r.log_probs, ref[rows, r.actions].clamp(EPS, 1 - EPS).log(), atol=1e-12)
    assert torch.equal(r.n_legal, masks.sum(1).int()) and r.flags.tolist() == [0, 0]
    # packed masks, bf16 logits and the (B, 9, 9, 139) shape are read alike
    p = sample_controlled(logits, _pack(masks), 9, controls=None)
    assert torch.equal(p.actions, r.actions) and torch.equal(p.probs, r.probs)
    lb = torch.randn(2, 9, 9, 139).to(torch.bfloat16)
    mb = torch.rand(2, 9 * 9 * 139) < 0.01
    mb[:, 3] = True
    s4 = sample_controlled(lb, mb, 1, controls=SamplingControls(0.5))
    s2 = sample_controlled(lb.float().reshape(2, -1), mb, 1, controls=SamplingControls(0.5))
    assert torch.equal(s4.actions, s2.actions) and torch.equal(s4.probs, s2.probs)


def test_temperature_scales_the_logits():
    logits, masks = _rows()
    for T in (0.5, 2.0):
        r = sample_controlled(logits, masks, 3, controls=SamplingControls(T))
        ref = torch.softmax((logits.double() / T).masked_fill(~masks, float("-inf")), dim=-1)
        assert torch.allclose(r.probs, ref, atol=1e-15, rtol=1e-12)


def test_greedy_and_top1_pick_the_argmax_ties_to_the_lower_index():
    logits, masks = _rows()
    masks[0, [7, 30]] = True
    logits[0, 7] = logits[0, 30] = 50.0                      # a duplicated maximum at two legal indices
    masks[0, 2] = False
    logits[0, 2] = 50.0                                      # ... and once at an illegal one
    want = logits.masked_fill(~masks, float("-inf")).argmax(dim=1)
    want[0] = 7
    for seed in (0, 1, 2):
        for c in (GREEDY, SamplingControls(1.0, top_k=1), SamplingControls(0.0, top_k=5)):
            r = sample_controlled(logits, masks, seed, controls=c)
            assert torch.equal(r.actions, want)
            assert torch.allclose(r.log_probs, torch.full((5,), math.log(1 - EPS), dtype=torch.float64))
            assert torch.equal(r.probs, torch.nn.functional.one_hot(want, 53).double())


def test_top_k_tie_straddling_the_cut_keeps_the_lower_index():
    logits = torch.full((1, 53), -5.0)
    masks = torch.ones(1, 53, dtype=torch.bool)
    logits[0, 40], logits[0, 10] = 3.0, 2.0
    logits[0, 20] = logits[0, 33] = 1.0                      # the third place is shared: 20 stays, 33 goes
    masks[0, 15] = False
    logits[0, 15] = 9.0
    r = sample_controlled(logits, masks, 4, controls=SamplingControls(1.0, top_k=3))
    assert torch.nonzero(r.probs[0]).reshape(-1).tolist() == [10, 20, 40]
    e = np.exp(np.array([2.0, 1.0, 3.0]) - 3.0)
    assert np.allclose(r.probs[0, [10, 20, 40]].numpy(), e / e.sum(), rtol=1e-13)
    assert int(r.n_legal[0]) == 52                           # every legal action, not |S|


def test_top_k_at_or_above_nlegal_is_no_cut():
    logits, masks = _rows()
    masks[2] = False
    masks[2, [4, 8, 12]] = True
    full = sample_controlled(logits, masks, 6, controls=SamplingControls(0.5))
    for k in (3, 4, 64):
        r = sample_controlled(logits[2:3], masks[2:3], 6, controls=SamplingControls(0.5, top_k=k))
        assert torch.equal(r.probs[0], full.probs[2])
    r64 = sample_controlled(logits, masks, 6, controls=SamplingControls(0.5, top_k=64))     # 53 actions at most
    assert torch.equal(r64.probs, full.probs) and torch.equal(r64.actions, full.actions)


def test_opening_switch_is_at_opening_plies():
    logits, masks = _rows()
    c = SamplingControls(temperature=0.0, opening_temperature=2.0, opening_plies=6)
    plies = torch.tensor([0, 5, 6, 7, 65535])
    r = sample_controlled(logits, masks, 8, controls=c, plies=plies)
    hot = sample_controlled(logits, masks, 8, controls=SamplingControls(2.0))
    cold = sample_controlled(logits, masks, 8, controls=GREEDY)
    for b, opening in enumerate([True, True, False, False, False]):
        want = hot if opening else cold
        assert torch.equal(r.probs[b], want.probs[b]) and r.actions[b] == want.actions[b], b
    as_int32 = sample_controlled(logits, masks, 8, controls=c, plies=plies.int())            # the column as an owner records it
    assert torch.equal(as_int32.probs, r.probs) and torch.equal(as_int32.actions, r.actions)
    with pytest.raises(ValueError, match="unsigned 32-bit"):
        sample_controlled(logits, masks, 8, controls=c, plies=plies - 1)
    late = sample_controlled(logits, masks, 8, controls=c)                  # no plies: past every opening
    assert torch.equal(late.probs, cold.probs)
    assert c.effective(5) == SamplingControls(2.0) and c.effective(6) == GREEDY and c.effective(None) == GREEDY


def test_rows_outside_the_table_take_their_first_legal_action():
    logits, masks = _rows()
    masks[:, :9] = False
    masks[1, 3] = True
    model_of = torch.tensor([0, -1, 2, 1, 0], dtype=torch.int32)
    r = sample_controlled(logits, masks, 5, controls=[SamplingControls(0.5), GREEDY], model_of=model_of)
    first = masks.int().argmax(dim=1)
    for b in (1, 2):
        assert r.actions[b] == first[b] and r.log_probs[b] == 0 and not r.probs[b].any()
    assert int(r.actions[1]) == 3
    assert torch.equal(r.probs[3], sample_controlled(logits, masks, 5, controls=GREEDY).probs[3])
    assert torch.equal(r.probs[0], sample_controlled(logits, masks, 5, controls=SamplingControls(0.5)).probs[0])


def test_row_without_a_legal_action_and_nan_are_flagged():
    logits, masks = _rows()
    masks[3] = False
    r = sample_controlled(logits, masks, 5, controls=SamplingControls(0.5, top_k=4))
    assert r.flags.tolist() == [0, 1] and r.actions[3] == 0 and r.log_probs[3] == 0 and int(r.n_legal[3]) == 0
    logits[0, 5] = float("nan")
    assert sample_controlled(logits, masks, 5, controls=None).flags.tolist() == [1, 1]


def test_a_malformed_table_row_reads_as_neutral():
    logits, masks = _rows()
    neutral = sample_controlled(logits, masks, 5, controls=None)
    for row in (struct.pack("<ffii", 0.5, 0.5, 0, 65), struct.pack("<ffii", -1.0, 1.0, 0, 0),
                struct.pack("<ffii", 1.0, float("nan"), 0, 3), struct.pack("<ffii", float("inf"), 1.0, 0, 0)):
        table = np.frombuffer(row, dtype=np.int32).reshape(1, 4).copy()
        r = sample_controlled(logits, masks, 5, controls=table)
        assert torch.equal(r.probs, neutral.probs) and torch.equal(r.actions, neutral.actions)


def _mix(x):
    m = (1 << 64) - 1
    x = (x + 0x9E3779B97F4A7C15) & m
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & m
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & m
    return x ^ (x >> 31)


@pytest.mark.parametrize("seed,row", [(0, 0), (0x1234_5678_9ABC_DEF0 - (1 << 62), 7), (-3, 299)])
def test_uniform_is_the_documented_mix(seed, row):
    m = (1 << 64) - 1
    u = (_mix((seed & m) ^ _mix((row + 0x5851F42D4C957F2D) & m)) >> 40) / 2.0 ** 24
    assert sample_uniform(seed, row) == u and 0.0 <= u < 1.0
    # the draw is the inverse CDF at that uniform, over the support in ascending action order
    logits, masks = _rows(B=300, seed=4)
    r = sample_controlled(logits, masks, seed, controls=SamplingControls(0.5, top_k=6))
    cdf = r.probs[row].cumsum(0)
    want = int(torch.nonzero(cdf > u * cdf[-1])[0])
    assert int(r.actions[row]) == want


def test_sample_controlled_refusals():
    logits, masks = _rows()
    with pytest.raises(ValueError, match="legal must be"):
        sample_controlled(logits, masks[:, :50], 1, controls=None)
    with pytest.raises(ValueError, match="float32 or bfloat16"):
        sample_controlled(logits.double(), masks, 1, controls=None)
    with pytest.raises(ValueError, match="expected 5 plies"):
        sample_controlled(logits, masks, 1, controls=None, plies=torch.zeros(4, dtype=torch.int64))
    with pytest.raises(ValueError, match="expected 5 model_of"):
        sample_controlled(logits, masks, 1, controls=None, model_of=torch.zeros(6, dtype=torch.int32))
    with pytest.raises(ValueError, match="expected 3"):
        sample_controlled(logits, masks, 1, controls=[GREEDY, NEUTRAL], num_models=3)
