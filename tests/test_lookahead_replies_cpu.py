"""The reply search of the lookahead on the CPU: the controls' fourth word, and the float64 restatement of the backed-up choice
on hand-made rows."""
import numpy as np
import pytest
import torch

from keisei_amd import _lib
from keisei_amd.training import (LookaheadControls, lookahead_active, lookahead_choose, lookahead_choose_replies,
                                 lookahead_reply_widths, lookahead_table)
from keisei_amd.training.lookahead import ERR_VALUE, arena_lookahead, arena_reply_width

WIN, DRAW, LOSS = [4.0, 0.0, -4.0], [0.0, 4.0, 0.0], [-4.0, 0.0, 4.0]       # value logits (W, D, L) of the side to move


def _p(vl):
    e = np.exp(np.asarray(vl, np.float64) - max(vl))
    return e / e.sum()


# ------------------------------------------------------------------ validation and the table word
def test_reply_width_is_validated_like_width_and_packed_into_word_3():
    assert LookaheadControls(3, 0.25).reply_width == 0 and LookaheadControls(3, 0.25, 4, 2).reply_width == 2
    assert LookaheadControls(3, reply_width=np.int64(8)).reply_width == 8
    for bad in (-1, 9, 1.0, True, "2", None):
        with pytest.raises(ValueError, match="reply_width"):
            LookaheadControls(3, reply_width=bad)
    with pytest.raises(ValueError, match="needs a width above 0"):
        LookaheadControls(0, reply_width=1)
    row = LookaheadControls(3, 0.5, 7, 2).row()
    assert row.dtype == np.int32 and row.tolist() == [3, int(np.float32(0.5).view(np.int32)), 7, 2]
    assert LookaheadControls(3, 0.5, 7).row().tolist()[3] == 0                 # the default is the word of today
    table = lookahead_table([LookaheadControls(3, 0.25, reply_width=2), LookaheadControls(2, 0.0, 4)], 2)
    assert table[:, 3].tolist() == [2, 0]


def test_the_table_readers_keep_their_shapes_and_the_reply_width_stands_beside_them():
    ctl = [LookaheadControls(3, 0.25, reply_width=2), LookaheadControls(2, 0.0, 4), LookaheadControls.OFF]
    table, width = arena_lookahead(ctl, 3, False)
    assert table.shape == (3, 4) and width == 3 and arena_reply_width(ctl, 3) == 2
    assert arena_lookahead(None, 3, False) == (None, 0) and arena_reply_width(None, 3) == 0
    assert arena_reply_width(LookaheadControls(2), 3) == 0
    widths, weights = lookahead_active(ctl, [0, 1, 2, -1, 3], [9, 9, 9, 9, 9])
    assert widths.tolist() == [3, 2, 0, 0, 0] and weights.tolist()[:2] == [0.25, 0.0]
    assert lookahead_reply_widths(ctl, [0, 1, 2, -1, 3]).tolist() == [2, 0, 0, 0, 0]
    assert lookahead_reply_widths(LookaheadControls(4, reply_width=5), [0, 0], num_models=1, reply_width=3).tolist() == [3, 3]
    # a table as it lies in device memory: word 3 outside [0, 8] reads as 0, and a row that is off has no replies
    raw = lookahead_table([LookaheadControls(3, reply_width=2)] * 4, 4)
    raw[1, 3], raw[2, 3], raw[3, 0] = 9, -1, 0
    assert lookahead_reply_widths(raw, [0, 1, 2, 3]).tolist() == [2, 0, 0, 0]
    # skip_plies plays no part at the reply level, and the env's reading of the row does not look at word 3
    assert lookahead_active(raw, [1, 2], [0, 0])[0].tolist() == [3, 3]


def test_the_abi_signatures_and_the_sizes():
    assert len(_lib._SIGS["ka_lookahead_fork_replies"].replace(" ", "")) == 24
    assert len(_lib._SIGS["ka_lookahead_choose_replies"].replace(" ", "")) == 22
    assert len(_lib._SIGS["ka_lookahead_fork"].replace(" ", "")) == 23 and len(_lib._SIGS["ka_lookahead_choose"].replace(" ", "")) == 15


# ------------------------------------------------------------------ the restatement on hand-made rows
def _rows(children, weight=0.0, priors=None):
    """One row from ``children``: per candidate ``(value_logits, reward, done, replies)``, a reply ``(value_logits, reward,
    done)``."""
    W, R = len(children), max(1, max(len(c[3]) for c in children))
    vl, rw, dn = torch.zeros(1, W, 3), torch.zeros(1, W), torch.zeros(1, W, dtype=torch.bool)
    nr = torch.zeros(1, W, dtype=torch.int32)
    gv, gr, gd = torch.zeros(1, W, R, 3), torch.zeros(1, W, R), torch.zeros(1, W, R, dtype=torch.bool)
    for j, (v, r, d, replies) in enumerate(children):
        vl[0, j], rw[0, j], dn[0, j], nr[0, j] = torch.tensor(v), r, d, len(replies)
        for k, (v2, r2, d2) in enumerate(replies):
            gv[0, j, k], gr[0, j, k], gd[0, j, k] = torch.tensor(v2), r2, d2
    p = torch.tensor([priors if priors is not None else [1.0 / W] * W], dtype=torch.float64)
    return lookahead_choose_replies(p, torch.tensor([W], dtype=torch.int32), vl, rw, dn, nr, gv, gr, gd, weight)


def test_a_mating_reply_makes_q_minus_one_exactly_and_the_blunder_is_refused():
    # candidate 0 looks winning at one ply and walks into a mate (the reply's mover gets +1); candidate 1 is a dull draw
    c = _rows([(LOSS, 0.0, False, [(WIN, 0.0, False), (DRAW, 0.0, False), (DRAW, 1.0, True)]),
               (DRAW, 0.0, False, [(DRAW, 0.0, False), (DRAW, 0.0, False)])])
    assert c.q[0, 0].item() == -1.0 and c.reply_slot[0].tolist() == [2, 0]
    assert c.slot.tolist() == [1] and c.one_ply_slot.tolist() == [0] and c.error == 0
    assert c.v[0, 0].tolist()[2] == -1.0 and c.v[0, 0, 0].item() == pytest.approx(_p(WIN)[0] - _p(WIN)[2], abs=1e-15)


def test_a_reply_into_a_repetition_makes_zero():
    c = _rows([(LOSS, 0.0, False, [(WIN, 0.0, True)])])        # a done grandchild's value logits are not looked at
    assert c.q[0, 0].item() == 0.0 and not np.signbit(c.q[0, 0].item()) and c.reply_slot[0, 0].item() == 0


def test_a_done_child_keeps_its_reward_and_a_child_without_replies_its_one_ply_q():
    c = _rows([(DRAW, 1.0, True, [(DRAW, 1.0, True)]),         # the mover's own mate: the "replies" of a restarted game count for nothing
               (LOSS, 0.0, False, []),
               (WIN, -1.0, True, [])])
    want = _p(LOSS)[2] - _p(LOSS)[0]
    assert c.q[0].tolist() == [1.0, pytest.approx(want, abs=1e-15), -1.0]
    assert c.reply_slot[0].tolist() == [-1, -1, -1] and c.slot.tolist() == [0]
    one = lookahead_choose(torch.full((1, 3), 1 / 3, dtype=torch.float64), torch.tensor([3]), torch.tensor([[DRAW, LOSS, WIN]]),
                           torch.tensor([[1.0, 0.0, -1.0]]), torch.tensor([[True, False, True]]), 0.0)
    assert torch.equal(one.q, c.q) and torch.equal(one.slot, c.slot)     # no reply anywhere: the one-ply choice


def test_ties_take_the_first_minimum_and_the_first_maximum():
    mid = [1.0, 0.0, -1.0]
    c = _rows([(DRAW, 0.0, False, [(WIN, 0.0, False), (mid, 0.0, False), (mid, 0.0, False)]),
               (DRAW, 0.0, False, [(mid, 0.0, False), (WIN, 0.0, False)]),
               (DRAW, 0.0, False, [(DRAW, 0.0, True), (DRAW, 0.0, False)])])      # 0 - 0 and P(W) - P(L) = 0 tie
    assert c.reply_slot[0].tolist() == [1, 0, 0]
    assert c.q[0, 0].item() == c.q[0, 1].item() > 0.0 == c.q[0, 2].item()
    assert c.slot.tolist() == [0]                                                 # candidates 0 and 1 tie: the lower slot
    # the prior breaks the tie only through its weight
    assert _rows([(DRAW, 0.0, False, [(mid, 0.0, False)]), (DRAW, 0.0, False, [(mid, 0.0, False)])], 0.5, [0.2, 0.8]).slot.tolist() == [1]
    assert _rows([(DRAW, 0.0, False, [(mid, 0.0, False)]), (DRAW, 0.0, False, [(mid, 0.0, False)])], 0.0, [0.2, 0.8]).slot.tolist() == [0]


def test_a_nan_grandchild_logit_gives_minus_inf_and_the_error_bit():
    c = _rows([(DRAW, 0.0, False, [(WIN, 0.0, False), ([0.0, float("nan"), 0.0], 0.0, False)]),
               (WIN, 0.0, False, [(LOSS, 0.0, False)])])
    assert np.isneginf(c.q[0, 0].item()) and c.reply_slot[0, 0].item() == 1 and c.error & ERR_VALUE
    assert c.slot.tolist() == [1]
    # behind a finished grandchild the logits are not looked at; a live child's own non-finite logit stays an error
    assert _rows([(DRAW, 0.0, False, [([float("inf"), 0.0, 0.0], 0.0, True)])]).error == 0
    assert _rows([([0.0, float("inf"), 0.0], 0.0, False, [(DRAW, 0.0, False)])]).error & ERR_VALUE


def test_the_sign_of_v_and_the_min_decide_these_rows():
    a, b = [2.0, 0.0, -2.0], [1.0, 0.0, -1.0]                  # grandchildren good for their side to move = the root mover
    pa, pb = _p(a)[0] - _p(a)[2], _p(b)[0] - _p(b)[2]
    assert pa > pb > 0
    # the sign: candidate 0's only reply leaves the mover better off than candidate 1's; with -v the order turns round
    c = _rows([(DRAW, 0.0, False, [(a, 0.0, False)]), (DRAW, 0.0, False, [(b, 0.0, False)])])
    assert c.slot.tolist() == [0] and c.q[0].tolist() == [pytest.approx(pa, abs=1e-15), pytest.approx(pb, abs=1e-15)]
    assert int(np.argmax([-pa, -pb])) == 1
    # the same through rewards: a reply that loses the game at once (reward -1 for the reply's mover) is +1 for the mover
    c = _rows([(DRAW, 0.0, False, [(DRAW, 1.0, True)]), (DRAW, 0.0, False, [(DRAW, -1.0, True)])])
    assert c.q[0].tolist() == [-1.0, 1.0] and c.slot.tolist() == [1]
    # min against max: candidate 0 has one very good and one bad reply, candidate 1 two middling ones
    lo = [-2.0, 0.0, 2.0]
    c = _rows([(DRAW, 0.0, False, [(a, 0.0, False), (lo, 0.0, False)]), (DRAW, 0.0, False, [(b, 0.0, False), (b, 0.0, False)])])
    assert c.slot.tolist() == [1] and c.reply_slot[0].tolist() == [1, 0]
    assert int(np.argmax([max(pa, -pa), max(pb, pb)])) == 0    # with max in the place of min the choice is the other one


def test_many_rows_with_their_own_weights_and_unused_slots():
    rng = np.random.default_rng(3)
    B, W, R = 40, 4, 3
    p = torch.from_numpy(rng.random((B, W)))
    nc = torch.from_numpy(rng.integers(0, W + 1, B).astype(np.int32))
    vl, gv = torch.from_numpy(rng.normal(size=(B, W, 3))), torch.from_numpy(rng.normal(size=(B, W, R, 3)))
    dn, gd = torch.from_numpy(rng.random((B, W)) < 0.2), torch.from_numpy(rng.random((B, W, R)) < 0.2)
    rw = torch.from_numpy(rng.integers(-1, 2, (B, W)).astype(np.float64)) * dn
    gr = torch.from_numpy(rng.integers(-1, 2, (B, W, R)).astype(np.float64)) * gd
    nr = torch.from_numpy(rng.integers(0, R + 1, (B, W)).astype(np.int32))
    pw = torch.from_numpy(rng.random(B))
    c = lookahead_choose_replies(p, nc, vl, rw, dn, nr, gv, gr, gd, pw)
    one = lookahead_choose(p, nc, vl, rw, dn, pw)
    assert torch.equal(c.one_ply_slot, one.slot) and c.error == 0
    for b in range(B):
        n = int(nc[b])
        assert (c.slot[b].item() == -1) == (n == 0) and np.isneginf(c.u[b, n:].numpy()).all()
        for j in range(n):
            k = int(nr[b, j])
            if dn[b, j] or k == 0:
                assert c.q[b, j].item() == one.q[b, j].item() and c.reply_slot[b, j].item() == -1
            else:
                v = c.v[b, j, :k].numpy()
                assert c.q[b, j].item() == v.min() and c.reply_slot[b, j].item() == int(np.argmin(v))
        if n:
            assert c.slot[b].item() == int(np.argmax(c.u[b, :n].numpy()))
    # reply_width 0 everywhere is the one-ply choice, to the bit
    zero = lookahead_choose_replies(p, nc, vl, rw, dn, torch.zeros_like(nr), gv, gr, gd, pw)
    assert torch.equal(zero.q, one.q) and torch.equal(zero.u, one.u) and torch.equal(zero.slot, one.slot)
