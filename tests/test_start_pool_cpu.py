"""The start-position pool without a GPU: SFEN parsing and formatting, the host restatement of the kernel's draw against
plain Python integers, the checks of a position that need no move generation, and the keyword plumbing of VecEnv and the
three device epochs."""
import inspect
from pathlib import Path

import numpy as np
import pytest

from keisei_amd import _lib, shogi_gym
from keisei_amd.shogi_gym import VecEnv, _static_position_errors, format_sfen, parse_sfen, start_pool_index
from keisei_amd.sl import prepare as prep
from keisei_amd.training import LeagueRollout, MatchArena, SelfPlayRollout
from keisei_amd.training.model_group import SEResNetGroup
from keisei_amd.training.models.se_resnet import SEResNetModel, SEResNetParams
from start_pool_helpers import HANDICAP, IN_CHECK, START, WHITE_TO_MOVE, draw_int

PROMOTED = "ln1g1g1nl/1ks2r3/1pppp1+Bpp/p4p3/9/2P1P4/PP1P1PPPP/2K1G2R1/LNSG3N+l b - 1"
HANDS = "ln1gk2nl/1r4gb1/p1pppp1pp/9/9/9/P1PPPP1PP/1B5R1/LN1GKG1NL w 2S2Psp 1"
TINY = dict(num_blocks=1, channels=32, se_reduction=8, global_pool_channels=16, policy_channels=8,
            value_fc_size=32, score_fc_size=16, obs_channels=50)


# ------------------------------------------------------------------ SFEN
@pytest.mark.parametrize("sfen", [START, PROMOTED, HANDS, WHITE_TO_MOVE], ids=["start", "promoted", "hands", "white"])
def test_sfen_round_trip(sfen):
    board, hands, side = parse_sfen(sfen)
    assert board.shape == (81,) and board.dtype == np.uint8 and hands.shape == (2, 7) and side in (0, 1)
    assert format_sfen(board, hands, side) == sfen
    b2, h2, s2 = parse_sfen(format_sfen(board, hands, side))
    assert np.array_equal(b2, board) and np.array_equal(h2, hands) and s2 == side


def test_sfen_fields_land_where_the_env_keeps_them():
    board, hands, side = parse_sfen(START)
    assert board[0] == 0x12 and board[4] == 0x18 and board[76] == 8 and board[9 + 1] == 0x17 and board[7 * 9 + 1] == 6
    assert not hands.any() and side == 0
    board, hands, side = parse_sfen(PROMOTED)
    assert board[2 * 9 + 6] == (6 | 0x20) and board[80] == (2 | 0x10 | 0x20)
    board, hands, side = parse_sfen(HANDS)
    assert side == 1 and hands[0].tolist() == [2, 0, 0, 2, 0, 0, 0] and hands[1].tolist() == [1, 0, 0, 1, 0, 0, 0]
    assert parse_sfen(START[:-2])[2] == 0                               # the move number is optional
    assert parse_sfen(IN_CHECK)[1][0, 4] == 1 and (parse_sfen(HANDICAP)[0] != 0).sum() == 39


@pytest.mark.parametrize("sfen, field", [
    ("lnsgkgsnl1/1r5b1/ppppppppp/9/9/9/PPPPPPPPP/1B5R1/LNSGKGSNL b - 1", "board"),        # ten files in a rank
    ("lnsgkgsnl/1r5b1/pppppppppp/9/9/9/PPPPPPPPP/1B5R1/LNSGKGSNL b - 1", "board"),
    ("lnsgkgsnl/1r5b1/ppppppppp/9/9/9/PPPPPPPPP/1B5R1/LNSGKGSNX b - 1", "board"),         # unknown letter
    ("lnsgkgsnl/1r5b1/ppppppppp/9/9/9/PPPPPPPPP/1B5R1/LNSGKGSNL x - 1", "side"),
    ("lnsgkgsnl/1r5b1/ppppppppp/9/9/9/PPPPPPPPP/1B5R1/LNSGKGSNL b 2 1", "hands"),
    ("lnsgkgsnl/1r5b1/ppppppppp/9/9/9/PPPPPPPPP/1B5R1 b - 1", "board"),
    ("lnsgkgsnl/1r5b1/ppppppppp/9/9/9/PPPPPPPPP/1B5R1/LNSG+KGSNL b - 1", "board"),
], ids=["ten-files", "ten-pawns", "letter", "side", "hands", "eight-ranks", "promoted-king"])
def test_malformed_sfen_names_the_string_and_the_field(sfen, field):
    with pytest.raises(ValueError) as e:
        parse_sfen(sfen)
    assert sfen in str(e.value) and f"{field} field" in str(e.value)


def test_get_sfen_uses_the_module_formatter():
    assert "format_sfen(" in inspect.getsource(VecEnv.get_sfen)


# ------------------------------------------------------------------ the draw
@pytest.mark.parametrize("K", [1, 3, 7, 2 ** 20])
def test_draw_restatement_equals_plain_integers(K):
    seeds = [0, 1, 7, 2 ** 31, 2 ** 63 + 12345, 2 ** 64 - 1]
    envs = np.array([0, 1, 2, 63, 64, 4095, 2 ** 20, 2 ** 31 + 5])
    games = np.array([0, 1, 2, 3, 100, 65535, 2 ** 31, 2 ** 32 - 1])
    for seed in seeds:
        got = start_pool_index(seed, envs[:, None], games[None, :], K)
        assert got.shape == (len(envs), len(games)) and got.dtype == np.int64
        want = np.array([[draw_int(seed, int(e), int(g), K) for g in games] for e in envs])
        assert np.array_equal(got, want)
        assert got.min() >= 0 and got.max() < K
    if K == 7:                                                          # every row is reached, and the seed matters
        many = start_pool_index(5, np.arange(64)[:, None], np.arange(8)[None, :], K)
        assert set(many.reshape(-1).tolist()) == set(range(K))
        assert not np.array_equal(many, start_pool_index(6, np.arange(64)[:, None], np.arange(8)[None, :], K))


def test_draw_refuses_an_empty_pool():
    with pytest.raises(ValueError, match="count"):
        start_pool_index(0, 0, 0, 0)


# ------------------------------------------------------------------ the checks that need no device
def _one(sfen):
    b, h, s = parse_sfen(sfen)
    return b[None].copy(), h.reshape(1, 14).copy(), np.array([s], np.uint8)


def test_static_checks_accept_the_fixture_positions():
    for sfen in (START, PROMOTED, HANDS, WHITE_TO_MOVE, IN_CHECK, HANDICAP):
        bad, _ = _static_position_errors(*_one(sfen))
        assert not bad.any(), sfen


def test_static_checks_name_the_first_failed_rule_per_row():
    rows = [_one(START) for _ in range(6)]
    rows[1][0][0, 40] = 9                                              # no piece byte
    rows[2][0][0, 76] = 0                                              # black king gone
    rows[3][1][0, 5] = 1                                               # a third bishop, in black's hand
    rows[4][0][0, 3 * 9] = 1 | 0x10                                    # a second white pawn on file 9 (and a 19th pawn)
    rows[4][0][0, 6 * 9 + 4] = 0
    b, h, s = (np.concatenate([r[i] for r in rows]) for i in range(3))
    bad, why = _static_position_errors(b, h, s)
    assert bad.tolist() == [False, True, True, True, True, False]
    assert "no piece" in why[1] and "black needs exactly one king" in why[2] and "more than 2 B" in why[3]
    assert "two unpromoted pawns" in why[4]


# ------------------------------------------------------------------ plumbing
def test_entry_points_are_bound_and_declared():
    names = set(_lib.exported_symbols())
    header = (Path(__file__).resolve().parent.parent / "include" / "keisei_amd.h").read_text()
    for n in ("ka_shogi_env_reset_pool", "ka_shogi_env_step_pool"):
        assert n in names and f"int {n}(" in header, n
    assert _lib._SIGS["ka_shogi_env_reset_pool"].replace(" ", "") == _lib._SIGS["ka_shogi_env_reset"].replace(" ", "")[:-1] + "ppp"
    assert _lib._SIGS["ka_shogi_env_step_pool"].replace(" ", "") == _lib._SIGS["ka_shogi_env_step"].replace(" ", "")[:-1] + "ppp"
    assert "0x706F6F6C" in header and shogi_gym.POOL_ROW_BYTES == 96


def test_keyword_plumbing():
    for cls in (VecEnv, SelfPlayRollout, LeagueRollout, MatchArena):
        p = inspect.signature(cls.__init__).parameters["start_pool_capacity"]
        assert p.default == 0 and p.kind is inspect.Parameter.KEYWORD_ONLY, cls.__name__
        if cls is not VecEnv:                                           # the epochs hand it to the VecEnv they own
            assert "start_pool_capacity=int(start_pool_capacity)" in inspect.getsource(cls.__init__), cls.__name__
    assert "opening_positions" in prep.__all__
    sig = inspect.signature(prep.opening_positions).parameters
    assert list(sig)[:4] == ["game_sources", "ply", "min_ply", "min_rating"] and sig["min_ply"].default == 40
    assert all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("max_positions", "device", "batch_envs"))
    with pytest.raises(ValueError, match="start_pool_capacity"):
        VecEnv(4, 10, "katago", "spatial", start_pool_capacity=-1)


def test_epochs_refuse_bad_pool_arguments_before_they_need_a_device():
    models = [SEResNetModel(SEResNetParams(**TINY)).eval() for _ in range(2)]
    group = SEResNetGroup(models)
    with pytest.raises(ValueError, match="features=True cannot be combined with start_pool_capacity"):
        MatchArena(group, 8, 4, 40, sync_every=2, features=True, start_pool_capacity=4)
    with pytest.raises(ValueError, match="start_pool_capacity must not be negative"):
        MatchArena(group, 8, 4, 40, sync_every=2, start_pool_capacity=-1)
    with pytest.raises(ValueError, match="GPU group"):                  # a valid pool argument gets as far as before
        MatchArena(group, 8, 4, 40, sync_every=2, start_pool_capacity=4)
    with pytest.raises(ValueError, match="start_pool_capacity must not be negative"):
        SelfPlayRollout(models[0], num_envs=8, max_ply=40, sync_every=8, start_pool_capacity=-1)
    with pytest.raises(ValueError, match="select_actions' loop"):
        SelfPlayRollout(models[0], num_envs=8, max_ply=40, sync_every=8, start_pool_capacity=4)
    with pytest.raises(ValueError, match="start_pool_capacity must not be negative"):
        LeagueRollout(models[0], models[1:], [1], num_envs=8, max_ply=40, sync_every=8, start_pool_capacity=-1)
