"""The host side of the mate-in-one check (keisei_amd/training/mate_search.py) and the positions the GPU tests stand on.

The positions of tests/mate_search_helpers.py are checked here against the C oracle alone: a badly built position fails in
this file first, so the GPU tests that compare csrc/mate.hip to the same oracle on them are not vacuous."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import mate_search_helpers as H
from keisei_amd import _lib
from keisei_amd.shogi_gym import parse_sfen
from keisei_amd.training import MatchArena, MateControls
from keisei_amd.training.mate_search import MAX_CHECKS, MateStats, arena_mate, mate_table, mate_words
from keisei_amd.training.model_group import SEResNetGroup
from keisei_amd.training.models.se_resnet import SEResNetModel, SEResNetParams
from oracle import shogi as S

ROOT = Path(__file__).resolve().parent.parent
TINY = dict(num_blocks=1, channels=32, se_reduction=8, global_pool_channels=16, policy_channels=8,
            value_fc_size=32, score_fc_size=16, obs_channels=50)


# ---------------------------------------------------------------------------------------------- the positions
def test_there_are_thirteen_positions_and_each_parses():
    assert len(H.NAMES) == 13 and set(H.WITH_MATE) | set(H.WITHOUT_MATE) | {"open"} == set(H.NAMES)
    for name in H.NAMES:
        board, hands, side = H.position(name)
        assert (board == S.KING).sum() == 1 and (board == (S.KING | S.WHITE)).sum() == 1, name


@pytest.mark.parametrize("name", H.WITH_MATE)
def test_positions_with_a_mate_have_one(name):
    checks, mates = H.expected(name)
    assert len(mates) >= 1 and set(mates) <= set(checks), (name, checks, mates)


@pytest.mark.parametrize("name", H.WITHOUT_MATE)
def test_positions_without_a_mate_have_none(name):
    checks, mates = H.expected(name)
    assert mates == (), (name, mates)


def test_the_start_position_has_no_checking_move():
    assert H.expected("start") == ((), ())


def test_the_pawn_drop_that_would_mate_is_absent_from_the_mask():
    board, hands, side = H.position("pawn_drop")
    checks, mates, legal = H.oracle_checks(board, hands, side)
    to = S.sq(1, 8)                                           # P*1b, on the head of the king on 1a
    drop = S.encode(0, to, drop=S.PAWN)
    env = H._scratch()
    env.set_state(0, board, hands, side)
    assert env.uchi_fu_zume(0, to, 0) and not legal[drop]
    assert legal[S.encode(0, S.sq(2, 7), drop=S.PAWN)]        # another pawn drop is legal: the hand is not the reason
    assert len(checks) == 2 and drop not in checks and mates == []


def test_the_discovering_bishop_does_not_attack_the_king_itself():
    board, hands, side = H.position("discovered")
    checks, mates = H.expected("discovered")
    env, hits = H._scratch(), 0
    king = int(np.flatnonzero(board == (S.KING | S.WHITE))[0])
    for a in mates:
        frm, to, promote, drop = S.decode(a)
        if board[frm] != S.BISHOP:
            continue
        env.set_state(0, board, hands.reshape(14), side)
        env.play(0, frm, to, bool(promote), drop)
        moved = int(board[frm]) | (S.PROM if promote else 0)
        hits += not env.piece_attacks(0, to, moved, king)
    assert hits >= 1


def test_the_double_check_is_a_mate():
    board, hands, side = H.position("double")
    king = int(np.flatnonzero(board == (S.KING | S.WHITE))[0])
    a = S.encode(S.sq(2, 4), S.sq(1, 5), promote=True)        # B5c-4b+: the horse checks and uncovers the rook on 5e
    env = H._scratch()
    env.set_state(0, board, hands.reshape(14), side)
    env.play(0, S.sq(2, 4), S.sq(1, 5), True, 0)
    assert env.piece_attacks(0, S.sq(1, 5), S.BISHOP | S.PROM, king) and env.piece_attacks(0, S.sq(4, 4), S.ROOK, king)
    assert a in H.expected("double")[1]


def test_the_promotion_twin_checks_and_only_the_promotion_mates():
    checks, mates = H.expected("promote")
    plain, dragon = S.encode(S.sq(2, 4), S.sq(2, 8)), S.encode(S.sq(2, 4), S.sq(2, 8), promote=True)
    assert plain in checks and dragon in checks and mates == (dragon,)


def test_the_knight_and_capture_and_evasion_mates_are_what_they_are_called():
    assert H.expected("knight")[1] == (S.encode(S.sq(4, 6), S.sq(2, 7)),)
    board, _, _ = H.position("capture")
    assert all(board[S.decode(a)[1]] != 0 for a in H.expected("capture")[1])            # every mate takes the pawn on 5b
    board, hands, side = H.position("evasion")
    env = H._scratch()
    env.set_state(0, board, hands.reshape(14), side)
    assert env.in_check(0, 0)
    _, mates, legal = H.oracle_checks(board, hands, side)
    assert len(mates) == 1 and board[S.decode(mates[0])[1]] == (S.GOLD | S.WHITE) and legal.sum() > 1


def test_white_to_move_positions_mirror_their_black_twins():
    for white, black in (("gold_drop_white", "gold_drop"), ("knight_white", "knight")):
        assert H.position(white)[2] == 1 and H.position(black)[2] == 0
        assert H.expected(white) == H.expected(black)          # the action index is in the mover's perspective


def test_the_open_position_has_many_checks_and_a_late_mate():
    checks, mates = H.expected("open")
    assert len(checks) > 16 and len(mates) == 1 and checks.index(mates[0]) >= 16          # rank above 16, counted from 1
    words = {a // 32 for a in checks}
    assert len(words) > 16 and min(words) < 64 and max(words) >= 256                       # both passes of 256 mask words
    assert H.expected_record(checks, mates, 16) == (list(checks[:16]), True, -1)
    assert H.expected_record(checks, mates, 64) == (list(checks), False, mates[0])


def test_the_pool_positions_are_mates_in_one_for_both_colours():
    sfens = H.pool_sfens()
    assert len(sfens) == 2 * len(H.POOL) and sorted(parse_sfen(s)[2] for s in sfens) == [0] * len(H.POOL) + [1] * len(H.POOL)
    env = H._scratch()
    for s in sfens:
        board, hands, side = parse_sfen(s)
        env.set_state(0, board, hands.reshape(14), side)
        assert not env.in_check(0, side) and not env.in_check(0, side ^ 1)
        assert H.oracle_checks(board, hands, side)[1], s


# ---------------------------------------------------------------------------------------------- controls and tables
def test_controls_are_validated_and_frozen():
    c = MateControls()
    assert (c.max_checks, c.skip_plies) == (16, 0) and MateControls.OFF == MateControls(0)
    assert MateControls(np.int64(64), np.int32(7)) == MateControls(64, 7)
    for bad in (dict(max_checks=-1), dict(max_checks=MAX_CHECKS + 1), dict(max_checks=True), dict(max_checks=4.0),
                dict(skip_plies=-1), dict(skip_plies=65536), dict(skip_plies="3")):
        with pytest.raises(ValueError, match=next(iter(bad))):
            MateControls(**bad)
    with pytest.raises(Exception):
        c.max_checks = 3


def test_table_layout():
    assert MateControls(5, 9).row().tolist() == [5, 9, 0, 0] and MateControls(5, 9).row().dtype == np.int32
    t = mate_table([MateControls(5, 9), MateControls.OFF, MateControls(64)], 3)
    assert t.dtype == np.int32 and t.tolist() == [[5, 9, 0, 0], [0, 0, 0, 0], [64, 0, 0, 0]]
    assert mate_table(None, 2).tolist() == [[0] * 4] * 2 and mate_table(MateControls(3), 2).tolist() == [[3, 0, 0, 0]] * 2
    assert mate_table({1: MateControls(8, 2)}, 3).tolist() == [[0] * 4, [8, 2, 0, 0], [0] * 4]
    for bad, K in (([MateControls()], 2), ({2: MateControls()}, 2), ([MateControls(), 3], 2), ("x", 1), (None, 0)):
        with pytest.raises(ValueError):
            mate_table(bad, K)
    assert mate_words(16) == 20 and MateStats() == MateStats(0, 0, 0, 0, 0)


def test_arena_reading_of_the_option():
    assert arena_mate(None, 2, True) == (None, 0)
    table, cap = arena_mate([MateControls(4), MateControls(32, 6)], 2, False)
    assert cap == 32 and table.tolist() == [[4, 0, 0, 0], [32, 6, 0, 0]]
    assert arena_mate(MateControls.OFF, 2, False)[1] == 0
    with pytest.raises(ValueError, match="collect=True"):
        arena_mate(MateControls(), 2, True)


def test_the_new_symbols_are_declared_and_exported():
    header = (ROOT / "include" / "keisei_amd.h").read_text()
    for name in ("ka_mate_words", "ka_mate_fork", "ka_mate_choose"):
        assert re.search(rf"^int {name}\(", header, re.M), name
        assert name in _lib.exported_symbols()
    lib = ctypes.CDLL(str(_lib.library_path()))
    assert [lib.ka_mate_words(w, 16) for w in range(5)] == [20, 4, 6, 64, -1]
    assert lib.ka_mate_words(0, 64) == 68 and lib.ka_mate_words(0, 65) == -1
    assert "mate.hip" in (ROOT / "keisei_amd" / "build.py").read_text()


def test_arena_with_mate_on_a_cpu_group_raises_like_the_lookahead():
    g = SEResNetGroup([SEResNetModel(SEResNetParams(**TINY)).eval() for _ in range(2)])
    with pytest.raises(ValueError, match="GPU group"):
        MatchArena(g, 8, 4, 40, sync_every=2, mate=MateControls())
    with pytest.raises(ValueError, match="GPU group"):
        MatchArena(g, 8, 4, 40, sync_every=2, graph=False, mate=[MateControls(4), MateControls.OFF])


def test_the_shared_field_checks():
    from test_lookahead_cpu import check_field_refusals
    check_field_refusals(MateControls, ints=(("max_checks", MAX_CHECKS), ("skip_plies", 65535), ("evasion_rows", 128),
                                             ("reply_checks", MAX_CHECKS)))
