"""Shared by tests/test_start_pool_cpu.py and tests/test_hip_start_pool.py: the start-position pool of the tests, built and
verified with the CPU oracle, the draw restated in plain Python integers, and the oracle side of a pooled run."""
from functools import lru_cache

import numpy as np

from keisei_amd.shogi_gym import format_sfen, parse_sfen, start_pool_index
from oracle import shogi as so

M64 = (1 << 64) - 1
START = "lnsgkgsnl/1r5b1/ppppppppp/9/9/9/PPPPPPPPP/1B5R1/LNSGKGSNL b - 1"
WHITE_TO_MOVE = "lnsgkgsnl/1r5b1/ppppppppp/9/9/2P6/PP1PPPPPP/1B5R1/LNSGKGSNL w - 1"
IN_CHECK = "4k4/9/9/9/4r4/9/9/9/4K4 b G 1"                    # the rook on 5e checks the king on 5i
HANDICAP = "lnsgkgsn1/1r5b1/ppppppppp/9/9/9/PPPPPPPPP/1B5R1/LNSGKGSNL w - 1"      # lance handicap: white moves first
MATE_SEARCH_SEED, HANDS_SEED = 10, 5


def mix_int(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def draw_int(seed: int, env: int, g: int, count: int) -> int:
    """The draw of include/keisei_amd.h in plain Python integers."""
    h = mix_int((seed & M64) ^ mix_int((((env << 32) | g) + 0x706F6F6C) & M64))
    return ((h >> 32) * count) >> 32


def _playable(board, hands, side) -> bool:
    env = so.OracleVecEnv(1, 500)
    env.set_state(0, board, hands, side)
    return env.legal_count(0) > 0 and not env.in_check(0, side ^ 1)


def _mating_action(board, hands, side):
    """An action of the side to move that leaves the other side without a legal move, or None: every legal move is
    played in a slot of its own of one probe env."""
    one = so.OracleVecEnv(1, 500)
    one.set_state(0, board, hands, side)
    legal = np.flatnonzero(one.observe(0)[1])
    probe = so.OracleVecEnv(len(legal), 500)
    for e in range(len(legal)):
        probe.set_state(e, board, hands, side)
    r = probe.step(legal.astype(np.int64))
    hit = np.flatnonzero(r["termination_reason"] == so.R_CHECKMATE)
    return int(legal[hit[0]]) if len(hit) else None


def _random_game_positions(seed: int, plies: int):
    """Positions of one seeded random oracle game, before every move."""
    env = so.OracleVecEnv(1, 500)
    _, mask = env.reset()
    rng = np.random.default_rng(seed)
    for _ in range(plies):
        board, hands, side, _ = env.state(0)
        yield board.copy(), hands.copy(), side
        r = env.step(np.array([rng.choice(np.flatnonzero(mask[0]))], np.int64))
        if r["terminated"][0] or r["truncated"][0]:
            return
        mask = r["legal_masks"]


@lru_cache(maxsize=None)
def mate_in_one():
    """(board, hands, side, mating action): the first position of seeded random oracle games from which a move mates."""
    for seed in range(MATE_SEARCH_SEED, MATE_SEARCH_SEED + 50):
        for i, (board, hands, side) in enumerate(_random_game_positions(seed, 400)):
            if i < 40 or not _playable(board, hands, side):
                continue
            a = _mating_action(board, hands, side)
            if a is not None:
                return board, hands, side, a
    raise AssertionError("no mate in one found")


@lru_cache(maxsize=None)
def both_hands():
    """The first position of a seeded random oracle game in which both hands hold pieces, one of them two of a kind."""
    for board, hands, side in _random_game_positions(HANDS_SEED, 400):
        if hands[0].sum() and hands[1].sum() and hands.max() > 1 and _playable(board, hands, side):
            return board, hands, side
    raise AssertionError("no position with both hands filled")


@lru_cache(maxsize=None)
def fixture_ply30():
    """The position after 30 moves of the first game of tests/golden/g15_games.sfen that is that long, replayed through
    the oracle."""
    from sl_prepare_helpers import fixture_games

    games, _ = fixture_games(None, max_moves=30)
    actions = next(g[0] for g in games if len(g[0]) == 30)
    env = so.OracleVecEnv(1, 500)
    _, mask = env.reset()
    for a in actions:
        assert mask[0, a]
        r = env.step(np.array([a], np.int64))
        assert not (r["terminated"][0] or r["truncated"][0])
        mask = r["legal_masks"]
    board, hands, side, ply = env.state(0)
    assert ply == 30
    return board.copy(), hands.copy(), side


MATE_INDEX = 5


@lru_cache(maxsize=None)
def pool7():
    """The seven start positions of the tests as (boards (7,81), hands (7,2,7), sides (7,)), each verified playable."""
    rows = [parse_sfen(START), parse_sfen(WHITE_TO_MOVE), parse_sfen(IN_CHECK), parse_sfen(HANDICAP), both_hands(),
            mate_in_one()[:3], fixture_ply30()]
    for b, h, s in rows:
        assert _playable(b, h, s), format_sfen(b, h, s)
    probe = so.OracleVecEnv(1, 500)
    probe.set_state(0, *rows[2])
    assert probe.in_check(0, rows[2][2])
    assert rows[1][2] == 1 and rows[3][2] == 1 and (rows[3][0] != 0).sum() == 39
    return (np.stack([r[0] for r in rows]).astype(np.uint8), np.stack([np.asarray(r[1]).reshape(2, 7) for r in rows]).astype(np.uint8),
            np.asarray([r[2] for r in rows], np.uint8))


def pool_observation(pool, idx: int, max_ply: int):
    """(observation, bool mask) of pool row idx at ply 0, by the oracle."""
    env = so.OracleVecEnv(1, max_ply)
    env.set_state(0, pool[0][idx], pool[1][idx], int(pool[2][idx]))
    return env.observe(0)


class PooledOracle:
    """OracleVecEnv whose finished games restart from the pool as the kernel draws them."""

    def __init__(self, n: int, max_ply: int, pool, seed: int):
        self.ref, self.n, self.pool, self.seed = so.OracleVecEnv(n, max_ply), n, pool, seed
        self.K = len(pool[2])
        self.games = np.zeros(n, np.int64)
        self.index = np.zeros(n, np.int64)
        self.drawn = []

    def _place(self, e: int):
        e = int(e)
        idx = int(start_pool_index(self.seed, e, int(self.games[e]), self.K))
        self.index[e] = idx
        self.drawn.append(idx)
        self.ref.set_state(e, self.pool[0][idx], self.pool[1][idx], int(self.pool[2][idx]))
        return self.ref.observe(e)

    def reset(self):
        obs, mask = self.ref.reset()
        self.games[:] = 0
        players = np.zeros(self.n, np.uint8)
        for e in range(self.n):
            obs[e], mask[e] = self._place(e)
            players[e] = self.pool[2][self.index[e]]
        return obs, mask, players

    def step(self, actions):
        r = self.ref.step(actions)
        for e in np.flatnonzero(r["terminated"] | r["truncated"]):
            self.games[e] += 1
            r["observations"][e], r["legal_masks"][e] = self._place(e)
            r["current_players"][e] = self.pool[2][self.index[e]]
        return r

    def ply(self, e: int) -> int:
        return self.ref.state(e)[3]


def choose_actions(po: PooledOracle, mask, rng, mate_index=None, mate_action=None):
    """Seeded random legal actions; the mating move where a game stands at the start of the mate-in-one position."""
    acts = np.array([rng.choice(np.flatnonzero(m)) for m in mask], dtype=np.int64)
    if mate_index is not None:
        for e in range(po.n):
            if po.index[e] == mate_index and po.ply(e) == 0:
                assert mask[e, mate_action]
                acts[e] = mate_action
    return acts
