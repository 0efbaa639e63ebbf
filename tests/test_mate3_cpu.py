"""The host side of the mate in three (keisei_amd/training/mate_search.py) and the positions the GPU tests stand on.

The positions of tests/mate3_helpers.py are checked here against the C oracle alone: what each is said to show -- which
checks prove, what the budget walk takes and skips, which cap cuts what -- fails in this file first, so the GPU tests that
compare csrc/mate3.hip to the same oracle on them are not vacuous."""
import ctypes
import re
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

import mate3_helpers as M
import mate_search_helpers as H
from keisei_amd import _lib
from keisei_amd.shogi_gym import parse_sfen
from keisei_amd.training import MatchArena, MateControls
from keisei_amd.training.mate_search import (MAX_CHECKS, MAX_EVASION_ROWS, Mate3Stats, MateStage, arena_mate, arena_mate3,
                                             mate3_reply_table, mate3_words, mate_table)
from keisei_amd.training.match_arena import RoundStats
from oracle import shogi as S

ROOT = Path(__file__).resolve().parent.parent


# ---------------------------------------------------------------------------------------------- the positions
def test_every_position_parses_has_no_mate_in_one_and_mirrors_its_twin():
    assert len(M.NAMES) == 12
    env = H._scratch()
    for name in M.NAMES:
        board, hands, side = M.position(name)
        assert (board == S.KING).sum() == 1 and (board == (S.KING | S.WHITE)).sum() == 1, name
        assert side == int(name.endswith("_white"))
        env.set_state(0, board, hands.reshape(14), side)
        assert not env.in_check(0, side) and not env.in_check(0, side ^ 1), name
        checks, mates, _ = H.oracle_checks(board, hands, side)
        assert checks and not mates, name
    for name in ("simple", "late", "interpose"):               # the action index is in the mover's perspective
        assert M.expected(name + "_white", 64, 128, 64) == M.expected(name, 64, 128, 64)


def test_simple_one_check_of_nine_proves_by_a_single_forced_evasion():
    x = M.expected("simple", 16, 32, 8)
    assert len(x.checks) == 9 and not x.truncated and x.active and x.skipped == 0
    assert x.proving == [3] and x.mate3 == 2499 and x.n[3] == 1
    assert x.choice(x.forked[0]) == 2499 and x.choice(2499) == 2499


def test_two_ways_the_lowest_is_played_and_an_incoming_one_stays():
    x = M.expected("two_ways", 16, 32, 8)
    assert len(x.checks) == 9 and [x.forked[j] for j in x.proving] == [3610, 3611]
    assert [x.n[j] for j in x.proving] == [3, 2]
    assert x.choice(x.forked[0]) == 3610 and x.choice(3611) == 3611 and x.choice(3610) == 3610


def test_none_no_check_proves():
    x = M.expected("none", 64, 128, 64)
    assert len(x.checks) == 6 and set(x.n) == {2, 3} and x.active and not x.proving and not x.cut and x.mate3 == -1
    assert x.choice(x.forked[2]) == x.forked[2]


def test_late_every_cap_cuts_it_off():
    x = M.expected("late", 16, 64, 16)
    assert x.n == [4, 3, 4, 5, 3, 5, 6, 4, 4] and x.rows == 38 and x.proving == [8] and x.mate3 == 5423 and not x.cut
    root = M.expected("late", 8, 64, 16)                       # the ninth check is behind max_checks
    assert not root.proving and root.truncated and root.cut and len(root.forked) == 8
    reply = M.expected("late", 16, 64, 8)                      # one reply's mate is its tenth checking move
    assert not reply.proving and reply.reply_truncated and not reply.truncated and reply.skipped == 0
    assert not M.expected("late", 16, 64, 9).proving and M.expected("late", 16, 64, 10).proving == [8]
    budget = M.expected("late", 16, 32, 16)                    # seven checks take 30 rows; the last two do not fit
    assert budget.first == [0, 4, 7, 11, 16, 19, 24, -1, -1] and budget.rows == 30 and budget.skipped == 2
    assert not budget.proving and budget.cut and not budget.truncated and not budget.reply_truncated


def test_interpose_the_budget_walk_goes_on_past_a_check_that_does_not_fit():
    x = M.expected("interpose", 64, 128, 64)
    assert len(x.checks) == 22 and x.n[2:9] == [16, 14, 12, 10, 8, 6, 4] and x.rows == 112 and not x.cut
    assert x.proving == [9, 16, 17] and x.mate3 == x.forked[9]
    small = M.expected("interpose", 64, 32, 64)
    assert small.first[:5] == [0, 3, 4, -1, 20] and small.rows == 32 and small.skipped == 18      # slot 3 skipped, slot 4 fits: 4 of 22 with rows
    assert all(small.first[j] < 0 for j in x.proving) and not small.proving and small.cut
    board, hands, side = M.position("interpose")
    assert hands[1].sum() > 0                                  # the defender has pieces in hand to drop in between


def test_pawn_drop3_the_only_third_ply_mate_is_a_pawn_drop():
    x = M.expected("pawn_drop3", 64, 128, 64)
    assert not x.proving and not x.cut and x.n[0] == 1
    board, hands, side = M.position("pawn_drop3")
    b, h, s, legal = M._after(board, hands, side, x.forked[0])
    b, h, s, legal = M._after(b, h, s, int(np.flatnonzero(legal)[0]))
    env = H._scratch()
    env.set_state(0, b, h.reshape(14), s)
    blocked = [to for to in range(81) if b[to] == 0 and env.uchi_fu_zume(0, to, s)]
    assert len(blocked) == 1 and not legal[S.encode(0, blocked[0], drop=S.PAWN, white=bool(s))]


def test_the_mate_in_one_positions_stay_depth_one():
    for name in H.WITH_MATE:
        x = M.expected3(*H.position(name), 64, 128, 64)
        assert x.mate1 == H.expected(name)[1][0] and not x.active and x.rows == 0 and x.choice(0) == x.mate1, name
    assert not M.expected3(*H.position("start"), 64, 128, 64).active


def test_the_pool_proves_at_its_caps_for_both_colours():
    sfens = M.pool_sfens()
    assert len(sfens) == 6 and sorted(parse_sfen(s)[2] for s in sfens) == [0, 0, 0, 1, 1, 1]
    for name in M.POOL:
        x = M.expected(name, *M.POOL_CAPS)
        assert x.proving and x.mate1 < 0, name
    assert not M.expected("interpose", *M.POOL_CAPS).proving


def test_the_record_words_of_the_helper():
    x = M.expected("two_ways", 16, 32, 8)
    w = M.expected_words(x, 16, x.forked[0])
    assert len(w) == mate3_words(16) == 38 and w[:6] == [1 | 2 | 4 | 16, 27, 3, 3610, 0b11000, 0]
    assert w[6:6 + 9] == x.n and w[6 + 9:6 + 16] == [-1] * 7 and w[22:22 + 9] == x.first
    assert M.expected_words(x, 16, 3611)[:4] == [1 | 2 | 16, 27, 4, 3611]


# ---------------------------------------------------------------------------------------------- controls and tables
def test_controls_are_validated_and_the_old_form_is_what_it_was():
    c = MateControls()
    assert (c.max_checks, c.skip_plies, c.evasion_rows, c.reply_checks) == (16, 0, 0, 0)
    assert c.row().tolist() == [16, 0, 0, 0] and MateControls(5, 9).row().tolist() == [5, 9, 0, 0]
    assert MateControls.OFF == MateControls(0) and MAX_EVASION_ROWS == 128
    d = MateControls(16, 0, np.int64(32), np.int32(8))
    assert (d.evasion_rows, d.reply_checks) == (32, 8) and d.row().tolist() == [16, 0, 32, 8] and d.row().dtype == np.int32
    assert MateControls(16, 0, 128, 64).row().tolist() == [16, 0, 128, 64]
    for bad in (dict(evasion_rows=-1, reply_checks=1), dict(evasion_rows=129, reply_checks=1), dict(evasion_rows=True, reply_checks=1),
                dict(evasion_rows=4.0, reply_checks=1), dict(reply_checks=-1, evasion_rows=1), dict(reply_checks=MAX_CHECKS + 1, evasion_rows=1),
                dict(reply_checks="3", evasion_rows=1)):
        with pytest.raises(ValueError, match=next(iter(bad))):
            MateControls(16, 0, **bad)
    for bad in (dict(evasion_rows=8), dict(reply_checks=8)):
        with pytest.raises(ValueError, match="both zero or both positive"):
            MateControls(16, 0, **bad)


def test_table_words_two_and_three():
    t = mate_table([MateControls(5, 9, 32, 8), MateControls.OFF, MateControls(64)], 3)
    assert t.dtype == np.int32 and t.tolist() == [[5, 9, 32, 8], [0, 0, 0, 0], [64, 0, 0, 0]]
    r = mate3_reply_table(t)
    assert r.dtype == np.int32 and r.tolist() == [[8, 0, 0, 0], [0] * 4, [0] * 4]
    # rows outside the ranges have depth three off: the third ply is given nothing to do
    assert mate3_reply_table(np.array([[16, 0, 129, 8], [16, 0, 32, 65], [16, 0, -1, 8], [16, 0, 32, 64]], np.int32))[:, 0].tolist() == [0, 0, 0, 64]
    assert mate3_words(16) == 38 and mate3_words(64) == 134 and Mate3Stats() == Mate3Stats(0, 0, 0, 0, 0, 0)
    assert RoundStats().mate3 is None


def test_arena_reading_of_the_option():
    assert arena_mate3(None, 2) == (0, 0) and arena_mate3(MateControls(16), 2) == (0, 0)
    assert arena_mate3([MateControls(4, 0, 32, 8), MateControls(32, 6, 64, 4)], 2) == (64, 8)
    assert arena_mate3({1: MateControls(8, 0, 16, 2)}, 3) == (16, 2)
    table, cap = arena_mate([MateControls(4, 0, 32, 8), MateControls(32, 6)], 2, False)          # its signature and pair stay
    assert cap == 32 and table.tolist() == [[4, 0, 32, 8], [32, 6, 0, 0]]
    with pytest.raises(ValueError, match="collect=True"):
        arena_mate(MateControls(16, 0, 32, 8), 2, True)
    with pytest.raises(ValueError, match="expected 2"):
        arena_mate3([MateControls()], 2)


def test_set_mate_refuses_what_is_above_the_built_sizes():
    arena = object.__new__(MatchArena)                         # the refusals come before anything touches the device
    arena.group, arena.collect, arena._ctl = [0, 1], False, None
    arena.ply = SimpleNamespace(stages={"mate": MateStage(mate_table(None, 2), 16, 32, 8)})    # the sizes built, no engine
    for controls, text in ((MateControls(17, 0, 32, 8), "max_checks 17"), (MateControls(16, 0, 33, 8), "evasion_rows 33"),
                           (MateControls(16, 0, 32, 9), "reply_checks 9")):
        with pytest.raises(ValueError, match=f"{text} is above the largest"):
            arena.set_mate(controls)
    arena.ply.stages["mate"] = MateStage(mate_table(None, 2), 16)    # built for the mate in one alone
    with pytest.raises(ValueError, match="evasion_rows 1 is above the largest"):
        arena.set_mate({0: MateControls(16, 0, 1, 1)})
    arena.collect = True
    with pytest.raises(ValueError, match="collect=True"):
        arena.set_mate(MateControls(16, 0, 32, 8))


def test_the_new_symbols_are_declared_and_exported():
    header = (ROOT / "include" / "keisei_amd.h").read_text()
    for name in ("ka_mate3_words", "ka_mate3_fork", "ka_mate3_gate", "ka_mate3_choose"):
        assert re.search(rf"^int {name}\(", header, re.M), name
        assert name in _lib.exported_symbols()
    lib = ctypes.CDLL(str(_lib.library_path()))
    assert [lib.ka_mate3_words(w, 16) for w in range(6)] == [38, 4, 7, 128, 64, -1]
    assert lib.ka_mate3_words(0, 64) == 134 and lib.ka_mate3_words(0, 65) == -1
    assert [lib.ka_mate_words(w, 16) for w in range(5)] == [20, 4, 6, 64, -1]            # the mate in one's, as before
    build = (ROOT / "keisei_amd" / "build.py").read_text()
    assert '"mate3.hip"' in build and '"mate.hip"' in build
