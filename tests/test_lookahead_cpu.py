"""The one-ply lookahead on the host: controls, table layout and the float64 restatement on hand-made rows."""
import math
import struct

import numpy as np
import pytest
import torch

from keisei_amd.shogi_gym import ACTION_SPACE, MASK_WORDS
from keisei_amd.training import (LookaheadControls, lookahead_active, lookahead_candidates, lookahead_choose,
                                 lookahead_table)
from keisei_amd.training.lookahead import arena_lookahead, lookahead_words

OFF = LookaheadControls.OFF
INF = float("inf")


# ------------------------------------------------------------------ controls and table
def test_controls_are_validated_and_frozen():
    c = LookaheadControls(3, 0.25, 8)
    assert (c.width, c.prior_weight, c.skip_plies) == (3, 0.25, 8)
    assert OFF == LookaheadControls() == LookaheadControls(0, 0.0, 0)
    with pytest.raises(Exception):
        c.width = 4
    for bad in (dict(width=-1), dict(width=9), dict(width=2.0), dict(width=True), dict(prior_weight=-0.1),
                dict(prior_weight=INF), dict(prior_weight=float("nan")), dict(prior_weight="1"), dict(prior_weight=1e39),
                dict(skip_plies=-1), dict(skip_plies=1.5), dict(skip_plies=1 << 20)):
        with pytest.raises(ValueError):
            LookaheadControls(**bad)
    assert LookaheadControls(np.int64(2), 1, np.int32(3)) == LookaheadControls(2, 1.0, 3)


def test_table_layout():
    t = lookahead_table([LookaheadControls(3, 0.5, 4), OFF, LookaheadControls(8)], 3)
    assert t.dtype == np.int32 and t.shape == (3, 4)
    assert t[0].tobytes() == struct.pack("<ifii", 3, 0.5, 4, 0)
    assert not t[1].any() and t[2].tolist() == [8, 0, 0, 0]
    assert np.array_equal(lookahead_table(LookaheadControls(2), 4), np.tile(LookaheadControls(2).row(), (4, 1)))
    assert not lookahead_table(None, 2).any()
    with pytest.raises(ValueError, match="expected 3"):
        lookahead_table([OFF, OFF], 3)
    with pytest.raises(ValueError, match="LookaheadControls"):
        lookahead_table([OFF, 3], 2)
    with pytest.raises(ValueError, match="at least one row"):
        lookahead_table(OFF, 0)
    assert lookahead_words(3) == 13 and lookahead_words(8) == 28


def test_arena_reading_of_the_option():
    assert arena_lookahead(None, 2, True) == (None, 0)
    table, width = arena_lookahead([LookaheadControls(2), LookaheadControls(5, 1.0)], 2, False)
    assert width == 5 and table.shape == (2, 4)
    assert arena_lookahead(OFF, 2, False)[1] == 0
    with pytest.raises(ValueError, match="collect=True"):
        arena_lookahead(OFF, 2, True)


def _raw_row(width, weight, skip):
    return np.frombuffer(struct.pack("<ifii", width, weight, skip, 0), dtype=np.int32)


def test_invalid_rows_read_as_off_and_skip_plies():
    table = np.stack([_raw_row(3, 0.5, 0), _raw_row(9, 0.0, 0), _raw_row(-1, 0.0, 0), _raw_row(2, -1.0, 0),
                      _raw_row(2, INF, 0), _raw_row(2, float("nan"), 0), _raw_row(2, 0.0, -5), _raw_row(4, 2.0, 6)])
    mo = [0, 1, 2, 3, 4, 5, 6, 7, -1, 8]
    w, pw = lookahead_active(table, mo)
    assert w.tolist() == [3, 0, 0, 0, 0, 0, 0, 4, 0, 0]
    assert pw[0] == 0.5 and pw[7] == 2.0
    # skip_plies: a position whose game ply is below it is left to the sampler
    w, _ = lookahead_active(table, [7, 7, 7, 0], plies=[0, 5, 6, 0])
    assert w.tolist() == [0, 0, 4, 3]
    # a width above the launch's is cut to it
    assert lookahead_active(table, [7, 0], width=2)[0].tolist() == [2, 2]
    ctl = [LookaheadControls(2, skip_plies=3), OFF]
    assert lookahead_active(ctl, [0, 1, 0], plies=[2, 9, 3])[0].tolist() == [0, 0, 2]


# ------------------------------------------------------------------ candidates
def _row(entries, B=1):
    """logits / bool mask rows with the given {action: logit} legal entries (one dict per row)"""
    logits = torch.full((B, ACTION_SPACE), 7.0)                  # illegal logits are large: they must not matter
    legal = torch.zeros(B, ACTION_SPACE, dtype=torch.bool)
    for b, d in enumerate(entries):
        for a, v in d.items():
            logits[b, a], legal[b, a] = v, True
    return logits, legal


def _pack(legal):
    B = legal.shape[0]
    bits = np.zeros((B, MASK_WORDS * 32), np.uint8)
    bits[:, :ACTION_SPACE] = legal.numpy()
    words = np.packbits(bits.reshape(B, MASK_WORDS, 32), axis=2, bitorder="little").view(np.uint32).reshape(B, MASK_WORDS)
    return torch.from_numpy(words.view(np.int32).copy())


def test_candidates_order_ties_and_priors():
    rows = [{5: 1.0, 31: 2.0, 32: 2.0, 900: 0.5, 11258: 2.0},     # ties across a word boundary and at the last action
            {40: -1.0, 41: 0.0},                                   # fewer legal moves than the width
            {77: 3.0},                                             # a single legal move
            {}]                                                    # no legal move
    logits, legal = _row(rows, 4)
    cand, prior, n = lookahead_candidates(logits, legal, 3)
    assert cand.tolist() == [[31, 32, 11258], [41, 40, -1], [77, -1, -1], [-1, -1, -1]]
    assert n.tolist() == [3, 2, 1, 0]
    z = np.array([1.0, 2.0, 2.0, 0.5, 2.0])
    p = np.exp(z - 2.0) / np.exp(z - 2.0).sum()
    assert np.allclose(prior[0].numpy(), [p[1], p[2], p[4]], rtol=1e-14)
    assert np.allclose(prior[1].numpy(), [1 / (1 + math.exp(-1)), math.exp(-1) / (1 + math.exp(-1)), 0], rtol=1e-14)
    assert prior[2].tolist() == [1.0, 0.0, 0.0] and prior[3].tolist() == [0.0, 0.0, 0.0]
    # packed rows give the same
    c2, p2, n2 = lookahead_candidates(logits, _pack(legal), 3)
    assert torch.equal(c2, cand) and torch.equal(p2, prior) and torch.equal(n2, n)
    # width 1 is the arg-max, lower action on a tie
    assert lookahead_candidates(logits, legal, 1)[0].reshape(-1).tolist() == [31, 41, 77, -1]


def test_a_legal_inf_or_nan_logit_is_never_a_candidate():
    logits, legal = _row([{3: -INF, 10: float("nan"), 64: 0.0, 65: -2.0}, {3: -INF, 4: float("nan")}], 2)
    cand, prior, n = lookahead_candidates(logits, legal, 4)
    assert cand.tolist() == [[64, 65, -1, -1], [-1, -1, -1, -1]] and n.tolist() == [2, 0]
    s = 1.0 + math.exp(-2.0)                                      # the NaN and the -inf weigh nothing
    assert np.allclose(prior[0].numpy(), [1 / s, math.exp(-2.0) / s, 0, 0], rtol=1e-14)
    assert not prior[1].any()


def test_candidates_refuse_other_shapes():
    logits, legal = _row([{1: 0.0}])
    with pytest.raises(ValueError, match="width"):
        lookahead_candidates(logits, legal, 0)
    with pytest.raises(ValueError, match="width"):
        lookahead_candidates(logits, legal, 9)
    with pytest.raises(ValueError, match="spatial action space"):
        lookahead_candidates(logits[:, :100], legal[:, :100], 2)
    with pytest.raises(ValueError, match="legal must be"):
        lookahead_candidates(logits, legal.int(), 2)


# ------------------------------------------------------------------ the choice
def _vl(q):
    """value logits (W, D, L) whose P(L) - P(W) is q (P(D) = 0.2)"""
    pl, pw = (0.8 + q) / 2, (0.8 - q) / 2
    return [math.log(pw), math.log(0.2), math.log(pl)]


def _choose(priors, qs, rewards=None, done=None, weight=0.0, n_cand=None):
    W = len(priors)
    vl = torch.tensor([[_vl(q) if q is not None else [0.0, 0.0, 0.0] for q in qs]], dtype=torch.float64)
    rw = torch.tensor([rewards if rewards is not None else [0.0] * W])
    dn = torch.tensor([done if done is not None else [False] * W])
    return lookahead_choose(torch.tensor([priors], dtype=torch.float64), torch.tensor([W if n_cand is None else n_cand]),
                            vl, rw, dn, weight)


def test_value_of_a_live_child_is_loss_minus_win_of_its_side_to_move():
    c = _choose([0.5, 0.3, 0.2], [-0.3, 0.6, 0.1])
    assert c.slot.tolist() == [1] and c.error == 0
    assert np.allclose(c.q.numpy(), [[-0.3, 0.6, 0.1]], atol=1e-15)
    assert np.allclose(c.u.numpy(), c.q.numpy())


def test_terminal_children():
    # a winning terminal child beats any live child
    assert _choose([0.6, 0.3, 0.1], [0.79, 0.79, None], rewards=[0, 0, 1.0], done=[False, False, True]).slot.tolist() == [2]
    # a losing terminal child loses to any live child
    assert _choose([0.6, 0.4], [None, -0.79], rewards=[-1.0, 0], done=[True, False]).slot.tolist() == [1]
    # a drawn terminal child counts as 0; the value logits of a finished child are not looked at
    c = lookahead_choose(torch.tensor([[0.5, 0.5]]), torch.tensor([2]), torch.tensor([[[INF, 0.0, 0.0], _vl(-0.1)]]),
                         torch.tensor([[0.0, 0.0]]), torch.tensor([[True, False]]), 0.0)
    assert c.slot.tolist() == [0] and c.error == 0 and c.q.tolist() == [[0.0, pytest.approx(-0.1)]]


def test_exact_ties_go_to_the_lower_slot():
    assert _choose([0.4, 0.3, 0.3], [0.25, 0.25, 0.25]).slot.tolist() == [0]
    assert _choose([0.4, 0.3, 0.3], [0.1, 0.25, 0.25]).slot.tolist() == [1]
    assert _choose([0.4, 0.3, 0.3], [None, None, None], rewards=[1.0, 1.0, 1.0], done=[True] * 3).slot.tolist() == [0]


def test_prior_weight_flips_a_choice_and_zero_does_not():
    priors, qs = [0.7, 0.2, 0.1], [0.10, 0.30, 0.20]
    assert _choose(priors, qs, weight=0.0).slot.tolist() == [1]
    assert _choose(priors, qs, weight=0.2).slot.tolist() == [1]           # 0.24, 0.34, 0.22
    c = _choose(priors, qs, weight=1.0)                                   # 0.80, 0.50, 0.30
    assert c.slot.tolist() == [0] and np.allclose(c.u.numpy(), [[0.8, 0.5, 0.3]])
    # one weight per row
    both = lookahead_choose(torch.tensor([priors, priors]), torch.tensor([3, 3]),
                            torch.tensor([[_vl(q) for q in qs]] * 2), torch.zeros(2, 3), torch.zeros(2, 3, dtype=torch.bool),
                            torch.tensor([0.0, 1.0]))
    assert both.slot.tolist() == [1, 0]


def test_fewer_candidates_than_the_width_and_none():
    # the unused slots are never chosen, whatever lies in them
    c = _choose([0.9, 0.1, 0.0, 0.0], [-0.5, -0.6, 0.7, 0.7], n_cand=2)
    assert c.slot.tolist() == [0] and c.u[0, 2:].tolist() == [-INF, -INF] and c.q[0, 2:].tolist() == [0.0, 0.0]
    assert _choose([1.0, 0.0, 0.0], [-0.7, 0.7, 0.7], n_cand=1).slot.tolist() == [0]       # a single legal move
    assert _choose([0.0, 0.0], [0.1, 0.2], n_cand=0).slot.tolist() == [-1]


def test_a_non_finite_value_logit_of_a_live_child_is_an_error_and_never_chosen():
    vl = torch.tensor([[[float("nan"), 0.0, 0.0], _vl(-0.7)], [[0.0, INF, 0.0], [0.0, 0.0, -INF]]], dtype=torch.float64)
    c = lookahead_choose(torch.tensor([[0.9, 0.1], [0.5, 0.5]]), torch.tensor([2, 2]), vl, torch.zeros(2, 2),
                         torch.zeros(2, 2, dtype=torch.bool), 5.0)
    assert c.error == 1 and c.slot.tolist() == [1, 0]
    assert c.q[0].tolist() == [-INF, pytest.approx(-0.7)] and c.q[1].tolist() == [-INF, -INF]


def test_choose_refuses_other_shapes():
    ok = dict(priors=torch.zeros(2, 3), n_cand=torch.zeros(2, dtype=torch.int32), child_value_logits=torch.zeros(2, 3, 3),
              child_rewards=torch.zeros(2, 3), child_done=torch.zeros(2, 3, dtype=torch.bool), prior_weight=0.0)
    lookahead_choose(**ok)
    for k, v in (("priors", torch.zeros(2, 9)), ("n_cand", torch.zeros(3)), ("child_value_logits", torch.zeros(2, 3)),
                 ("child_rewards", torch.zeros(2, 2)), ("prior_weight", -1.0), ("prior_weight", INF)):
        with pytest.raises(ValueError):
            lookahead_choose(**dict(ok, **{k: v}))


# ------------------------------------------------------------------ the shared table reader and field checks
def check_table_of(make_table, what, one, two):
    """``table_of`` for one kind of table (the other ``*_cpu.py`` files call this for theirs): ``one`` a controls object,
    ``two`` a sequence of two."""
    from keisei_amd.training._forked_rows import table_of
    assert np.array_equal(table_of(one, None, make_table, what), make_table(one, 1))
    assert np.array_equal(table_of(one, 3, make_table, what), make_table(one, 3))
    assert np.array_equal(table_of(two, None, make_table, what), make_table(two, 2))
    raw = make_table(two, 2)
    for given in (raw, torch.from_numpy(raw)):                 # a table as it lies on the device: unchanged
        got = table_of(given, None, make_table, what)
        assert got.dtype == np.int32 and got.shape == (2, 4) and np.array_equal(got, raw)
        assert np.array_equal(table_of(given, 2, make_table, what), raw)
    for bad in (raw.astype(np.int64), raw.view(np.float32), raw[:, :3], raw.reshape(-1), raw[:0]):
        with pytest.raises(ValueError, match=f"a {what} table is a \\(K, 4\\) int32 array"):
            table_of(bad, None, make_table, what)
    with pytest.raises(ValueError, match="expected a table of 3 rows, got 2"):
        table_of(raw, 3, make_table, what)


def check_field_refusals(make, ints=(), weights=()):
    """``make(**{field: value})`` refuses what ``check_int`` / ``check_weight`` refuse, under the field's own name.
    ``ints``: ``(field, hi)`` pairs, ``weights``: field names."""
    for field, hi in ints:
        for bad in (True, 1.0, hi + 1, -1):
            with pytest.raises(ValueError, match=f"{field} must be an integer in"):
                make(**{field: bad})
    for field in weights:
        for bad, text in ((True, "be finite and >= 0"), (float("nan"), "be finite and >= 0"), (-0.5, "be finite and >= 0"),
                          (3.1e38, "fit a float32")):
            with pytest.raises(ValueError, match=f"{field} must {text}"):
                make(**{field: bad})


def test_the_shared_table_reader_and_field_checks():
    from keisei_amd.training._forked_rows import check_int, check_weight
    check_table_of(lookahead_table, "lookahead", LookaheadControls(3, 0.25), [LookaheadControls(3, 0.25, 2, 1), LookaheadControls()])
    check_field_refusals(lambda **kw: LookaheadControls(**dict({"width": 1}, **kw)),
                         ints=(("width", 8), ("skip_plies", 65535), ("reply_width", 8)), weights=("prior_weight",))
    assert check_int("n", np.int64(7), 1, 7) == 7 and type(check_int("n", np.int64(7), 1, 7)) is int
    assert check_weight("w", 2) == 2.0 and type(check_weight("w", 2)) is float and check_weight("w", 3.0e38) == 3.0e38
    for bad in (True, 2.0, 8, 0, "3", None):
        with pytest.raises(ValueError, match=r"n must be an integer in \[1, 7\]"):
            check_int("n", bad, 1, 7)
    for bad in (float("inf"), "1", None):
        with pytest.raises(ValueError, match="w must be finite and >= 0"):
            check_weight("w", bad)
