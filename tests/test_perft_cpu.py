"""The host side of perft (keisei_amd/perft.py) and the numbers the GPU tests stand on: the table of
tests/perft_helpers.py is checked here against the C oracle alone, so the GPU tests that hold csrc/perft.hip to the same
numbers are not vacuous; the Python walk they compare columns with is checked against ``so_perft`` where both apply."""
import ctypes
import re
from pathlib import Path

import numpy as np
import pytest

import perft_helpers as P
from keisei_amd import _lib, build
from keisei_amd.perft import COLUMNS, MAX_DEPTH, MAX_MOVES, MAX_ROWS, PerftResult, check_perft_args, perft_plan_host

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("name", P.NAMES)
def test_the_table_is_the_oracles_perft_and_so_is_its_mirror(name):
    sfen, counts = P.TABLE[name]
    for d, want in enumerate(counts, start=1):
        if want > 1_000_000:                                     # (the one entry that takes the C oracle seconds: once, below)
            continue
        assert P.so_perft(sfen, d) == want, (name, d)
        assert P.so_perft(P.MIRRORS[name], d) == want, (name, d, "mirror")


def test_the_largest_entry_of_the_table():
    sfen, counts = P.TABLE["mid_drops"]
    assert P.so_perft(sfen, 3) == counts[2] == 4809015


def test_the_mirrors_are_other_positions_with_the_other_side_to_move():
    for name, (sfen, _) in P.TABLE.items():
        assert P.MIRRORS[name] != sfen and P.MIRRORS[name].split()[1] != sfen.split()[1], name
        back, want = P.parse_sfen(P.mirror_sfen(P.MIRRORS[name])), P.parse_sfen(sfen)
        assert all(np.array_equal(x, y) for x, y in zip(back, want)), name


@pytest.mark.parametrize("name", P.SMALL)
def test_the_env_walk_equals_so_perft_where_only_mates_end_games(name):
    sfen, counts = P.TABLE[name]
    for s in (sfen, P.MIRRORS[name]):
        by_depth = P.env_perft(s, len(counts))
        assert by_depth.shape == (len(counts), 4) and by_depth.dtype == np.uint64
        assert by_depth[:, 0].tolist() == list(counts), name
        assert by_depth[:, 2].tolist() == [0] * len(counts), name          # no game ended other than by mate
        # a mated node has no successors: the nodes of the next depth come from the others
        assert (by_depth[:, 1] <= by_depth[:, 0]).all() and (by_depth[:, 3] <= by_depth[:, 0]).all()


def test_the_small_set_covers_mates_and_checks():
    assert set(P.SMALL) == {"evasion", "pawn_drop"}
    assert P.env_perft(P.TABLE["evasion"][0], 3)[:, 1].sum() > 0         # K x g and more: mates inside the tree
    assert P.env_perft(P.TABLE["evasion"][0], 3)[:, 3].sum() > 0
    gold = P.env_perft(P.GOLD_HEAD, 2)
    assert gold[0, 1] > 0 and gold[:, 2].sum() == 0                      # the gold on the head mates at depth 1


def test_the_env_walk_under_a_move_limit_of_two():
    by_depth = P.env_perft(P.START, 3, 2)
    assert by_depth[:, 0].tolist() == [30, 900, 0]                       # every game ends with the second move
    assert by_depth[:, 2].tolist() == [0, 900, 0] and by_depth[:, 1].sum() == 0


@pytest.mark.parametrize("moves, cursor, cap, want", P.PLAN_CASES)
def test_plan_host_edges(moves, cursor, cap, want):
    taken, children, blocking, offsets = perft_plan_host(moves, cursor, cap)
    assert (taken, children, blocking) == want
    assert len(offsets) == taken
    run = np.maximum(np.asarray(moves[cursor:cursor + taken], np.int64), 0)
    assert offsets == (np.cumsum(run) - run).tolist()
    assert children == int(run.sum()) <= cap
    if cursor + taken < len(moves):                                      # the prefix is the longest: the next does not fit
        assert children + max(moves[cursor + taken], 0) > cap


def test_plan_host_never_loops_on_a_parent_that_cannot_fit():
    taken, children, blocking, _ = perft_plan_host([MAX_MOVES + 1], 0, MAX_MOVES)
    assert taken == 0 and blocking == 0                                   # the caller raises on `blocking`, it does not retry
    assert perft_plan_host([MAX_MOVES], 0, MAX_MOVES)[:3] == (1, MAX_MOVES, -1)


def test_plan_host_random_against_a_restatement():
    rng = np.random.default_rng(5)
    moves = rng.integers(0, MAX_MOVES + 1, 4096).tolist()
    cursor, chunks = 0, 0
    while cursor < len(moves):
        taken, children, blocking, offsets = perft_plan_host(moves, cursor, 2048)
        csum = np.cumsum(moves[cursor:])
        assert taken == int((csum <= 2048).sum()) > 0 and blocking == -1
        assert children == int(csum[taken - 1]) and offsets[0] == 0
        cursor, chunks = cursor + taken, chunks + 1
    assert chunks > 4096 * 250 // 2048


def test_argument_validation():
    assert check_perft_args(1, 1) == (1, 1) and check_perft_args(np.int64(MAX_DEPTH), MAX_ROWS) == (MAX_DEPTH, MAX_ROWS)
    for depth in (0, -1, MAX_DEPTH + 1, 2.0, "3", None, True):
        with pytest.raises(ValueError, match="depth"):
            check_perft_args(depth, 16384)
    for rows in (0, -5, MAX_ROWS + 1, 1024.0, None, True):
        with pytest.raises(ValueError, match="rows"):
            check_perft_args(3, rows)
    with pytest.raises(ValueError, match="cursor"):
        perft_plan_host([1, 2], 3, 8)
    with pytest.raises(ValueError, match="cap"):
        perft_plan_host([1, 2], 0, 0)
    assert MAX_DEPTH == 8 and MAX_MOVES == 593 and COLUMNS == ("nodes", "mates", "ended_otherwise", "checks")
    r = PerftResult(np.zeros(1, np.uint64), np.zeros((1, 2, 4), np.uint64), 0)
    assert r.chunks == 0 and r.by_depth.shape == (1, 2, 4)


def test_the_public_methods_exist_with_the_documented_defaults():
    import inspect

    from keisei_amd.shogi_gym import VecEnv
    sig = inspect.signature(VecEnv.perft)
    assert [p.default for p in list(sig.parameters.values())[2:]] == [16384, True]
    assert inspect.signature(VecEnv.perft_divide).parameters["rows"].default == 16384
    for fn in (VecEnv.perft, VecEnv.perft_divide):
        assert "ValueError" in fn.__doc__ or "as `perft`" in fn.__doc__
    assert "other than by checkmate" in VecEnv.perft.__doc__ and "no successors" in VecEnv.perft.__doc__


def test_the_new_symbols_are_declared_exported_and_bound():
    header = (ROOT / "include" / "keisei_amd.h").read_text()
    for name in ("ka_perft_words", "ka_perft_tally", "ka_perft_plan", "ka_perft_fork"):
        assert re.search(rf"^int {name}\(", header, re.M), name
        assert name in _lib.exported_symbols()
    lib = ctypes.CDLL(str(_lib.library_path()))
    assert [lib.ka_perft_words(w) for w in range(6)] == [4, 3, MAX_MOVES, MAX_ROWS, MAX_DEPTH, -1]
    for name in ("ka_perft_tally", "ka_perft_plan", "ka_perft_fork"):
        assert getattr(lib, name) is not None
    assert "perft.hip" in build.SOURCES
