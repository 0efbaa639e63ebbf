"""Shared by tests/test_sl_prepare_cpu.py and tests/test_hip_sl_prepare.py: the g15 fixture's games as replay batches and
the comparison of a replay's buffer with the fixture."""
from pathlib import Path

import numpy as np

from keisei_amd.sl import prepare as prep
from keisei_amd.sl.dataset import RECORD_SIZE
from keisei_amd.sl.parsers import CSAParser, SFENParser, is_standard_start
from oracle import shogi as so

GOLDEN = Path(__file__).resolve().parent / "golden"
FILES = (GOLDEN / "g15_games.sfen", GOLDEN / "g15_games.csa")
RANKS = "abcdefghi"


def obs_checksum(obs) -> np.uint64:
    """The fixture's 64-bit checksum of an observation (tools/make_sl_prepare_golden.py)."""
    w = np.ascontiguousarray(obs, dtype=np.float32).reshape(-1).view(np.uint32).astype(np.uint64)
    k = np.arange(w.size, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0xD1B54A32D192ED03)
    with np.errstate(over="ignore"):
        return np.uint64((w * k).sum(dtype=np.uint64))


def parsed_records():
    return list(SFENParser().parse(FILES[0])) + list(CSAParser().parse(FILES[1]))


def fixture_games(g, max_moves=None, repeat=1):
    """The fixture's standard-start games as ``(actions, outcome, host reason)`` and their fixture indices."""
    max_moves = int(g.np("max_moves")) if max_moves is None else max_moves
    games, index = [], []
    for k, rec in enumerate(parsed_records()):
        if is_standard_start(rec.start):
            actions, why = prep._encode_game(rec, max_moves)
            games.append((actions, prep._OUTCOME[rec.outcome], why))
            index.append(k)
    return games * repeat, index * repeat


def oracle_replay(max_moves):
    return lambda batch: prep._replay_host(batch, so.OracleVecEnv(batch.num_envs, max_moves))


def check_against_golden(g, games, index, batch, buf, valid_len, reason):
    """buffer / valid_len / reason of a replay of ``games`` (fixture indices ``index``) against the fixture, exactly."""
    gv, gr, pos_game = g.np("valid_len"), g.np("reason"), g.np("pos_game")
    raw = buf.view(np.uint8).reshape(-1, RECORD_SIZE)
    kept = prep._kept_rows(batch, valid_len)
    assert (raw[~kept] == 0xA5).all(), "a row of a cut move was written"
    for e in range(batch.num_envs):
        k = index[batch.order[e]]
        final = reason[e] if reason[e] else games[batch.order[e]][2]
        assert (int(valid_len[e]), int(final)) == (int(gv[k]), int(gr[k])), (g.np("tags")[k], valid_len[e], final, gv[k], gr[k])
        rows = buf[int(batch.row_of[e]):int(batch.row_of[e]) + int(valid_len[e])]
        sel = pos_game == k
        assert np.array_equal(rows["policy"], g.np("pos_policy")[sel]), g.np("tags")[k]
        assert np.array_equal(rows["value"], g.np("pos_value")[sel]), g.np("tags")[k]
        want = g.np("pos_material")[sel].astype(np.float32) / np.float32(76.0)
        assert np.array_equal(rows["score"].view(np.uint32), want.view(np.uint32)), g.np("tags")[k]
        sums = np.array([obs_checksum(o) for o in rows["obs"]], dtype=np.uint64)
        assert np.array_equal(sums, g.np("pos_checksum")[sel]), g.np("tags")[k]




def shifted_observations(batch, buf, valid_len):
    """A copy of the buffer in which every kept record but a game's last holds the observation of the game's NEXT record:
    what a replay gives that observes after the move."""
    out = buf.copy()
    for e in range(batch.num_envs):
        lo, n = int(batch.row_of[e]), int(valid_len[e])
        if n > 1:
            out["obs"][lo:lo + n - 1] = buf["obs"][lo + 1:lo + n]
    return out
