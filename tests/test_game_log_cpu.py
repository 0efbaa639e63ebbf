"""The game log without a GPU: action <-> USI, the .sfen export against SFENParser, the host restatement of the log
kernels on a hand-written script, the argument errors of the two owners."""
import ctypes

import numpy as np
import pytest

from keisei_amd import _lib
from keisei_amd.shogi_gym import ACTION_SPACE, SpatialActionMapper, parse_sfen
from keisei_amd.sl.parsers import START_SFEN, GameOutcome, SFENParser, is_standard_start
from keisei_amd.sl.prepare import usi_to_action
from keisei_amd.training import MatchArena, SelfPlayRollout, game_log_host, write_sfen_games
from keisei_amd.training.game_log import RecordedGame, usi_of
from keisei_amd.training.model_group import SEResNetGroup
from keisei_amd.training.models.se_resnet import SEResNetModel, SEResNetParams

TINY = dict(num_blocks=1, channels=32, se_reduction=8, global_pool_channels=16, policy_channels=8,
            value_fc_size=32, score_fc_size=16, obs_channels=50)
WHITE_SFEN = "lnsgkgsnl/1r5b1/ppppppppp/9/9/2P6/PP1PPPPPP/1B5R1/LNSGKGSNL w - 1"


def test_entry_points_are_exported():
    lib = ctypes.CDLL(str(_lib.library_path()))
    for name in ("ka_gamelog_words", "ka_gamelog_begin", "ka_gamelog_step", "ka_gamelog_seat"):
        assert hasattr(lib, name), name
        assert name in _lib.exported_symbols(), name
    assert _lib.query("ka_gamelog_words", 0, 512) == 12 + 24 + 256
    assert _lib.query("ka_gamelog_words", 0, 7) == 12 + 24 + 4
    assert _lib.query("ka_gamelog_words", 1, 0) == 4
    assert _lib.query("ka_gamelog_words", 99, 0) == -1


# ---------------------------------------------------------------------------------------------- action <-> USI
def test_every_decodable_action_round_trips_through_usi():
    mapper, seen = SpatialActionMapper(), 0
    for white in (False, True):
        for a in range(ACTION_SPACE):
            try:
                mapper.decode(a, white)
            except ValueError:
                continue
            seen += 1
            assert usi_to_action(usi_of(a, white), white) == a, (a, white)
    assert seen > 2 * 4000


def _board(r, c):
    return r * 9 + c


@pytest.mark.parametrize("white, action, usi", [
    # black: a square is row * 9 + column, row 0 = rank a, column 0 = file 9; slot = direction * 8 + distance - 1
    (False, _board(6, 2) * 139 + 0, "7g7f"),                            # pawn push, north by one
    (False, _board(7, 1) * 139 + 64 + 1 * 8 + 4, "8h3c+"),              # bishop north-east by five, promoting
    (False, _board(8, 1) * 139 + 128, "8i9g"),                          # knight jump to the left
    (False, _board(8, 1) * 139 + 130, "8i7g"),                          # knight jump to the right
    (False, _board(4, 4) * 139 + 132, "P*5e"),
    (False, _board(4, 4) * 139 + 133, "L*5e"),
    (False, _board(4, 4) * 139 + 134, "N*5e"),
    (False, _board(4, 4) * 139 + 135, "S*5e"),
    (False, _board(4, 4) * 139 + 136, "G*5e"),
    (False, _board(4, 4) * 139 + 137, "B*5e"),
    (False, _board(0, 8) * 139 + 138, "R*1a"),
    # white: the same indices on the board turned by 180 degrees (square q -> 80 - q)
    (True, _board(6, 2) * 139 + 0, "3c3d"),
    (True, _board(8, 1) * 139 + 128, "2a1c"),
    (True, _board(8, 1) * 139 + 130, "2a3c"),
    (True, _board(8, 7) * 139 + 129, "8a7c+"),                          # the left jump (in the mover's view), promoting
    (True, _board(0, 8) * 139 + 138, "R*9i"),
])
def test_usi_of_hand_picked_moves(white, action, usi):
    assert usi_of(action, white) == usi
    assert usi_to_action(usi, white) == action


# ---------------------------------------------------------------------------------------------- .sfen export
def _game(sfen, usi, winner, **kw):
    board, hands, side = parse_sfen(sfen)
    actions = np.asarray([usi_to_action(m, bool((side + i) & 1)) for i, m in enumerate(usi)], np.uint16)
    base = dict(reason=1, truncated=False, carried=False, env=0, black=-1, white=-1, end_ply=len(usi) - 1, game_number=0)
    base.update(kw)
    return RecordedGame(np.asarray(board, np.uint8).reshape(81), np.asarray(hands, np.uint8).reshape(2, 7), int(side), actions,
                        winner, **base)


def test_write_sfen_games_is_read_back_by_the_parser(tmp_path):
    standard = _game(START_SFEN, ["7g7f", "3c3d", "8h2b+", "3a2b", "B*5e"], 0, black=3, white=5, reason=1)
    from_white = _game(WHITE_SFEN, ["3c3d", "2g2f", "2b8h+"], 1, reason=1)
    drawn = _game(START_SFEN, ["2g2f", "8c8d"], 2, truncated=True, reason=5)
    empty = _game(START_SFEN, [], 2)
    assert standard.is_standard_start and not from_white.is_standard_start
    assert from_white.start_sfen() == WHITE_SFEN and from_white.start_side == 1
    assert (standard.outcome, from_white.outcome, drawn.outcome) == (GameOutcome.WIN_BLACK, GameOutcome.WIN_WHITE, GameOutcome.DRAW)
    path = tmp_path / "games.sfen"
    games = [standard, from_white, empty, drawn]
    assert write_sfen_games(path, games, metadata=[{"event": "round 7"}, {"event": "x"}, {}, {"event": "y"}]) == 3
    back = list(SFENParser().parse(path))
    assert len(back) == 3                                       # the game without a move is not written
    for rec, g in zip(back, [standard, from_white, drawn]):
        assert [m.move_usi for m in rec.moves] == g.usi_moves()
        assert rec.outcome == g.outcome
        assert is_standard_start(rec.start) == g.is_standard_start
        assert rec.metadata["reason"] == str(g.reason)
    assert back[0].start == "startpos" and back[1].start == WHITE_SFEN
    assert back[0].metadata == {"result": "win_black", "black": "3", "white": "5", "reason": "1", "event": "round 7"}
    assert back[1].metadata == {"result": "win_white", "reason": "1", "event": "x"}
    assert back[2].metadata == {"result": "draw", "reason": "5", "event": "y"}
    assert [usi_to_action(m.move_usi, bool((1 + i) & 1)) for i, m in enumerate(back[1].moves)] == from_white.actions.tolist()
    with pytest.raises(ValueError, match="no digit"):
        write_sfen_games(path, [standard], metadata={"elo1": "5"})
    with pytest.raises(ValueError, match="metadata names"):
        write_sfen_games(path, [standard], metadata=[{}, {}])


# ---------------------------------------------------------------------------------------------- the host restatement
def _script():
    """Eight plies, three envs.  Env 1 finishes at plies 3 and 7, envs 0 and 2 at ply 7; env 2 is not live at plies 2, 3."""
    plies = []
    for t in range(8):
        z = lambda dt: np.zeros(3, dt)  # noqa: E731
        ply = dict(actions=np.asarray([t + 1, 101 + t, 201 + t]), rewards=z(np.float32), terminated=z(bool), truncated=z(bool),
                   pre_players=np.asarray([t & 1, t & 1, t & 1], np.uint8), reason=z(np.uint8), live=np.asarray([0, 1, 0], np.int32))
        plies.append(ply)
    plies[2]["live"][2] = plies[3]["live"][2] = -1
    plies[3]["terminated"][1], plies[3]["rewards"][1], plies[3]["reason"][1] = True, 1.0, 1       # the mover, white, wins
    plies[7]["truncated"][0], plies[7]["reason"][0] = True, 5                                     # cut at max_ply: a draw
    plies[7]["terminated"][1], plies[7]["rewards"][1], plies[7]["reason"][1] = True, -1.0, 1      # white moved and lost
    plies[7]["terminated"][2], plies[7]["rewards"][2], plies[7]["reason"][2] = True, 1.0, 1       # white moved and won
    return plies


def _summary(g):
    return (g.env, g.actions.tolist(), g.winner, g.reason, g.truncated, g.carried, g.end_ply, g.game_number)


def test_game_log_host_on_a_hand_written_script():
    log = game_log_host(_script(), num_envs=3, max_ply=8, capacity=8)
    assert log.cursor.tolist() == [4, 0, 8, 0]
    games = log.games()
    assert [_summary(g) for g in games] == [
        (1, [101, 102, 103, 104], 1, 1, False, False, 3, 0),
        (0, [1, 2, 3, 4, 5, 6, 7, 8], 2, 5, True, False, 7, 0),                # ply 7: env 0 before env 1 before env 2
        (1, [105, 106, 107, 108], 0, 1, False, False, 7, 1),
        (2, [201, 202, 203, 204, 205, 206, 207, 208], 1, 1, False, True, 7, 0),
    ]
    assert all(g.is_standard_start and (g.black, g.white) == (-1, -1) for g in games)
    assert log.meta[:, :3].tolist() == [[0, 0, 1], [0, 0, 2], [0, 0, 1]]     # rows emptied, flags cleared, games counted

    small = game_log_host(_script(), num_envs=3, max_ply=8, capacity=2)
    assert small.cursor.tolist() == [2, 2, 8, 0]                              # the third and the fourth game are dropped
    assert [_summary(g) for g in small.games()] == [_summary(g) for g in games[:2]]
    assert np.array_equal(small.records, log.records[:2])


def test_game_log_host_pairs_seat_and_stall():
    plies = _script()
    for p in plies:
        p["live"] = None
    pairs = np.asarray([7, 9, 0, 0], np.int32)                   # one pair of three envs: 7 plays black, 9 white
    plies[5]["seat"] = (np.asarray([[0, 9, 7, 4]], np.int32), 1, 3)          # every game in progress is inherited
    plies[3]["n_legal"] = np.asarray([3, 3, 0], np.int32)        # an env of the group has no legal action: no commit
    log = game_log_host(plies, num_envs=3, max_ply=8, capacity=8, pairs=pairs, pair_stride=4, envs_per_pair=3)
    games = log.games()
    assert [(g.env, g.carried, g.black, g.white, g.game_number) for g in games] == [(0, True, 7, 9, 0), (1, True, 7, 9, 1),
                                                                                   (2, True, 7, 9, 0)]
    assert games[1].actions.tolist() == [105, 106, 107, 108]     # the uncommitted game was still cleared at its end


# ---------------------------------------------------------------------------------------------- argument errors
def test_owner_argument_errors():
    model = SEResNetModel(SEResNetParams(**TINY)).eval()
    with pytest.raises(ValueError, match="game_log must not be negative"):
        SelfPlayRollout(model, num_envs=8, max_ply=40, sync_every=8, game_log=-1)
    with pytest.raises(ValueError, match="GPU"):
        SelfPlayRollout(model, num_envs=8, max_ply=40, sync_every=8, game_log=16)
    group = SEResNetGroup([model])
    with pytest.raises(ValueError, match="game_log must not be negative"):
        MatchArena(group, 8, 4, 40, sync_every=2, game_log=-1)
    with pytest.raises(ValueError, match="GPU group"):
        MatchArena(group, 8, 4, 40, sync_every=2, game_log=16)
