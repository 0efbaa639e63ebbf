"""The game log with per-env players (ka_gamelog_step_env) and the games in progress (ka_gamelog_peek) without a GPU: the
host restatement on a hand-written script, the decoding of the new header word, and what refuses an unfinished game."""
import ctypes

import numpy as np
import pytest

from keisei_amd import _lib
from keisei_amd.sl.prepare import dataset_from_recorded_games
from keisei_amd.training import game_log_host, write_sfen_games
from keisei_amd.training.game_log import (CARRIED, HEAD_WORDS, START_WORDS, HostGameLog, RecordedGame, games_from_records,
                                          record_words)

E, MAX_PLY, K, PLIES = 3, 5, 2, 8
IDS = np.asarray([100, 7, 9], np.int32)                          # the learner, opponent 0, opponent 1


def _script():
    """Eight plies of three envs, K = 2, max_ply 5 (odd).  The state rows differ per ply, so a start slot shows when it
    was loaded.
      env 0  game 0: plies 0-2; the learner's side changes at ply 1 (0 -> 1); terminated at ply 2, the mover (black) wins
             game 1: plies 3-4 with side 0, opponent 1 (a change BETWEEN two games); truncated at ply 4
             game 2: plies 5-7 with opponent index 5 (outside [0, K)); terminated at ply 7, a draw
      env 1  game 0: plies 0-3; the opponent changes at ply 2 (0 -> 1); terminated at ply 3 with n_legal == 0: not committed
             game 1: plies 4-7; terminated at ply 7, the mover (white) loses
      env 2  game 0: plies 0-6, seven moves against max_ply 5; truncated at ply 6"""
    rng = np.random.default_rng(0)
    side = np.asarray([[0, 1, 1, 0, 0, 0, 0, 0], [1] * 8, [0] * 8], np.uint8).T
    opp = np.asarray([[0, 0, 0, 1, 1, 5, 5, 5], [0, 0, 1, 1, 0, 0, 0, 0], [1] * 8], np.int32).T
    tm = np.zeros((PLIES, E), bool)
    tr = np.zeros((PLIES, E), bool)
    rw = np.zeros((PLIES, E), np.float32)
    nl = np.full((PLIES, E), 30, np.int32)
    tm[2, 0], rw[2, 0] = True, 1.0
    tr[4, 0] = True
    tm[7, 0] = True
    tm[3, 1], rw[3, 1], nl[3, 1] = True, 1.0, 0
    tm[7, 1], rw[7, 1] = True, -1.0
    tr[6, 2] = True
    pre = np.asarray([[0, 1, 0, 0, 1, 0, 1, 0], [0, 1, 0, 1, 0, 1, 0, 1], [0, 1, 0, 1, 0, 1, 0, 1]], np.uint8).T
    plies = []
    for t in range(PLIES):
        plies.append(dict(actions=np.asarray([1000 + 10 * t + e for e in range(E)], np.int64), rewards=rw[t], terminated=tm[t],
                          truncated=tr[t], pre_players=pre[t], reason=np.asarray([t % 5 + 1] * E, np.uint8), n_legal=nl[t],
                          state=rng.integers(0, 256, (E, 96), dtype=np.uint8), side=side[t], opp=opp[t]))
    return plies, rng.integers(0, 256, (E, 96), dtype=np.uint8)


def _moves(e, lo, hi):
    return [1000 + 10 * t + e for t in range(lo, hi)]


def _start(g):
    return np.concatenate([g.start_board, g.start_hands.reshape(14), [g.start_side]]).astype(np.uint8)


def test_entry_points_are_exported():
    lib = ctypes.CDLL(str(_lib.library_path()))
    for name in ("ka_gamelog_step_env", "ka_gamelog_peek"):
        assert hasattr(lib, name), name
        assert name in _lib.exported_symbols(), name


def test_the_script_through_the_host_log():
    plies, start = _script()
    log = game_log_host(plies, num_envs=E, max_ply=MAX_PLY, capacity=8, start_state=start, ids=IDS)
    assert log.cursor.tolist() == [5, 0, PLIES, 0]
    games = log.games()
    # (ply, env) order; env 1's first game had an env without a legal action and is not committed
    assert [(g.env, g.game_number, g.end_ply) for g in games] == [(0, 0, 2), (0, 1, 4), (2, 0, 6), (0, 2, 7), (1, 1, 7)]
    a, b, long_one, c, d = games
    # a side change mid-game: carried, and the players who ended it (the learner white, opponent 0)
    assert (a.black, a.white, a.learner_side, a.carried, a.winner, a.truncated) == (7, 100, 1, True, 0, False)
    assert a.actions.tolist() == _moves(0, 0, 3) and a.learner_result == "loss" and a.finished
    assert np.array_equal(_start(a)[:95], start[0, :95])
    # a change between two games sets nothing
    assert (b.black, b.white, b.learner_side, b.carried, b.truncated, b.winner) == (100, 9, 0, False, True, 2)
    assert b.actions.tolist() == _moves(0, 3, 5) and b.learner_result == "draw"
    assert np.array_equal(_start(b)[:95], plies[2]["state"][0, :95])            # loaded when game 0 finished
    # an opponent index outside [0, K)
    assert (c.black, c.white, c.learner_side, c.carried, c.winner) == (100, -1, 0, False, 2)
    assert c.actions.tolist() == _moves(0, 5, 8)
    # the game after the uncommitted one: its opponent change happened in the game before
    assert (d.black, d.white, d.learner_side, d.carried, d.winner) == (7, 100, 1, False, 0)
    assert d.actions.tolist() == _moves(1, 4, 8) and d.learner_result == "loss"
    assert np.array_equal(_start(d)[:95], plies[3]["state"][1, :95])
    # seven moves against max_ply 5
    assert long_one.actions.tolist() == _moves(2, 0, 5) and long_one.truncated and not long_one.carried
    assert (long_one.black, long_one.white, long_one.learner_side) == (100, 9, 0)
    # header word 9, and the zero upper half of the last move word of an odd game
    assert log.records[:5, 9].tolist() == [2, 1, 1, 1, 2]
    assert log.records[:5, 10:12].tolist() == [[0, 0]] * 5
    moves_at = HEAD_WORDS + START_WORDS
    assert int(log.records[0, moves_at + 1]) == 1020 and int(log.records[2, moves_at + 2]) == 1042
    # every game is over: the tags are cleared where a game finished at the last ply
    assert log.meta[:, 3].tolist() == [0, 0, ((1 << 1) | 0) + 1]
    assert log.meta[:, 2].tolist() == [3, 2, 1]


def test_an_opponent_change_in_the_middle_of_a_committed_game_is_carried():
    plies, start = _script()
    plies[3]["n_legal"][1] = 30                                   # env 1's first game now counts
    log = game_log_host(plies, num_envs=E, max_ply=MAX_PLY, capacity=8, start_state=start, ids=IDS)
    g = [g for g in log.games() if (g.env, g.game_number) == (1, 0)][0]
    assert (g.black, g.white, g.learner_side, g.carried) == (9, 100, 1, True)        # opponent 1 ended it
    assert g.winner == 1 and g.learner_result == "win" and g.actions.tolist() == _moves(1, 0, 4)


def test_a_full_log_drops_whole_games_and_counts_them():
    plies, start = _script()
    full = game_log_host(plies, num_envs=E, max_ply=MAX_PLY, capacity=8, start_state=start, ids=IDS)
    log = game_log_host(plies, num_envs=E, max_ply=MAX_PLY, capacity=1, start_state=start, ids=IDS)
    assert log.cursor.tolist() == [1, 4, PLIES, 0]
    assert np.array_equal(log.records[0, :HEAD_WORDS + START_WORDS + 2], full.records[0, :HEAD_WORDS + START_WORDS + 2])
    assert np.array_equal(log.meta, full.meta) and np.array_equal(log.starts, full.starts)


def test_pairs_and_per_env_players_do_not_mix():
    log = HostGameLog(E, MAX_PLY, 2)
    plies, start = _script()
    log.begin(start)
    p = plies[0]
    args = (p["state"], p["actions"], p["rewards"], p["terminated"], p["truncated"], p["pre_players"], p["reason"])
    with pytest.raises(ValueError, match="not both"):
        log.step(*args, pairs=np.zeros((E, 2), np.int32), pair_stride=2, side=p["side"], opp=p["opp"], ids=IDS)
    with pytest.raises(ValueError, match="not both"):
        log.peek(pairs=np.zeros((E, 2), np.int32), pair_stride=2, side=p["side"], opp=p["opp"], ids=IDS)


@pytest.mark.parametrize("upto", [1, 2, 4, 6])
def test_peek_is_the_finished_record_so_far_and_changes_nothing(upto):
    plies, start = _script()
    full = game_log_host(plies, num_envs=E, max_ply=MAX_PLY, capacity=8, start_state=start, ids=IDS)
    finished = {(g.env, g.game_number): g for g in full.games()}
    log = game_log_host(plies[:upto], num_envs=E, max_ply=MAX_PLY, capacity=8, start_state=start, ids=IDS)
    before = [b.copy() for b in (log.rows, log.meta, log.starts, log.records, log.cursor)]
    nxt = plies[upto]
    out = np.full((E + 2, record_words(MAX_PLY)), 0x5A5A5A5A, np.int32)
    rows = log.peek([2, 1, 0, E, -1], side=nxt["side"], opp=nxt["opp"], ids=IDS, ply_counter=upto, out=out)
    assert rows is out
    for b, a in zip(before, (log.rows, log.meta, log.starts, log.records, log.cursor)):
        assert np.array_equal(a, b)
    peeked = games_from_records(rows[:3])
    assert [g.env for g in peeked] == [2, 1, 0]
    for g in peeked:
        assert not g.finished and g.winner == -1 and g.reason == 0 and not g.truncated and g.end_ply == upto
        assert g.learner_result is None and g.learner_side == int(nxt["side"][g.env])
        n = int(log.meta[g.env, 0])
        assert len(g.actions) == n
        words = (n + 1) // 2
        assert (rows[[2, 1, 0].index(g.env), HEAD_WORDS + START_WORDS + words:] == 0x5A5A5A5A).all()
        if n % 2:
            assert int(rows[[2, 1, 0].index(g.env), HEAD_WORDS + START_WORDS + words - 1]) >> 16 == 0
        end = finished.get((g.env, g.game_number))
        if end is not None:
            assert g.actions.tolist() == end.actions[:n].tolist()
            assert np.array_equal(_start(g), _start(end))
    # the rows of indices outside [0, E)
    for row in rows[3:]:
        assert row[:HEAD_WORDS].tolist() == [-1, 0, -1, 0, 0, -1, -1, upto, 0, 0, 0, 0]
        assert (row[HEAD_WORDS:HEAD_WORDS + START_WORDS] == 0).all() and (row[HEAD_WORDS + START_WORDS:] == 0x5A5A5A5A).all()
    # the other two sources of the players
    pairs = np.asarray([[3, 4, 0, 0]], np.int32)
    named = games_from_records(log.peek(pairs=pairs, pair_stride=4, envs_per_pair=E))
    assert all((g.black, g.white, g.learner_side) == (3, 4, None) for g in named) and [g.env for g in named] == [0, 1, 2]
    nobody = games_from_records(log.peek())
    assert all((g.black, g.white, g.learner_side) == (-1, -1, None) for g in nobody)
    assert [g.actions.tolist() for g in nobody] == [g.actions.tolist() for g in reversed(peeked)]


def test_peek_carries_the_flag_the_last_move_set():
    plies, start = _script()
    log = game_log_host(plies[:2], num_envs=E, max_ply=MAX_PLY, capacity=8, start_state=start, ids=IDS)
    rows = log.peek(side=plies[2]["side"], opp=plies[2]["opp"], ids=IDS)
    assert rows[:, 4].tolist() == [CARRIED, 0, 0]                 # env 0's side changed at ply 1


def test_an_old_style_record_decodes_without_a_learner():
    plies, start = _script()
    for p in plies:
        del p["side"], p["opp"]
    log = game_log_host(plies, num_envs=E, max_ply=MAX_PLY, capacity=8, start_state=start)
    assert (log.records[:5, 9] == 0).all() and (log.meta[:, 3] == 0).all()
    games = log.games()
    assert len(games) == 5
    for g in games:
        assert g.learner_side is None and g.finished is True and g.learner_result is None
        assert (g.black, g.white) == (-1, -1) and not g.carried
    g = RecordedGame(games[0].start_board, games[0].start_hands, 0, games[0].actions, 0, 1, False, False, 0, -1, -1, 2, 0)
    assert g.finished is True and g.learner_side is None          # the fields before this change still build a game


def test_an_unfinished_game_is_not_written_and_not_replayed(tmp_path):
    plies, _ = _script()
    log = game_log_host(plies[:2], num_envs=E, max_ply=MAX_PLY, capacity=8, ids=IDS)
    live = games_from_records(log.peek(side=plies[2]["side"], opp=plies[2]["opp"], ids=IDS))
    assert len(live) == E and all(not g.finished for g in live)
    with pytest.raises(ValueError, match="in progress"):
        write_sfen_games(tmp_path / "live.sfen", live)
    assert not (tmp_path / "live.sfen").exists()
    with pytest.raises(ValueError, match="in progress"):
        dataset_from_recorded_games(live)
    with pytest.raises(ValueError, match="no outcome"):
        live[0].outcome
