"""Shared by tests/test_perft_cpu.py and tests/test_hip_perft.py: the known perft answers (computed with the C oracle's
``so_perft``, ``OracleVecEnv.perft``, at ``max_ply`` 500), their colour-swapped images, and a perft under the env's game
rules walked on the oracle env (``oracle_env_perft``), which is what csrc/perft.hip is held to column for column.

In none of the trees of ``TABLE`` can a game end other than by mate -- the history is empty and a fourfold repetition needs
at least 12 plies, an impasse needs ten pieces of each side in the far camps and no position here has more than 6, the move
limit is far away -- so the env's perft must equal these numbers; the tests still assert the "ended otherwise" column."""
from functools import lru_cache

import numpy as np

from keisei_amd.shogi_gym import parse_sfen
from mate_search_helpers import POSITIONS, START, mirror_sfen
from oracle import shogi as S
from oracle.shogi import OracleVecEnv

# name -> (SFEN, (perft 1, perft 2, ...))
TABLE = {
    "start": (START, (30, 900, 25470, 719731)),
    "max593": ("R8/2K1S1SSk/4B4/9/9/9/9/9/1L1L1L3 b RBGSNLP3g3n17p 1", (593, 105677)),
    "mid_hands": ("ln1g1g1nl/1ks2r3/1pppp1bpp/p3spp2/9/P1P1SP1PP/1PBPP1P2/2KS3R1/LN1G1G1NL b - 1", (41, 1475, 60175)),
    "mid_drops": ("l6nl/5+P1gk/2np1S3/p1p4Pp/3P2Sp1/1PPb2P1P/P5GS1/R8/LN4bKL w RGgsn5p 1", (207, 28684, 4809015)),
    "open": ("4K4/9/9/9/9/9/5B3/9/8k b RBGL 1", (323, 596, 154604)),
    "evasion": ("4k4/4g4/4KG3/9/9/9/9/9/9 b - 1", (4, 24, 223)),
    "pawn_drop": ("7nk/9/8G/9/9/9/9/9/4K4 b P 1", (78, 156, 2526)),
}
NAMES = tuple(TABLE)
MIRRORS = {name: mirror_sfen(sfen) for name, (sfen, _) in TABLE.items()}
GOLD_HEAD = POSITIONS["gold_head"][0]
SMALL = tuple(n for n in NAMES if sum(TABLE[n][1]) <= 3000)      # the trees oracle_env_perft walks in the CPU test

# ka_perft_plan's edge lists: (moves, cursor, cap, (taken, children, blocking))
PLAN_CASES = [
    ([0], 0, 8, (1, 0, -1)),                                     # a parent with no moves is taken and has no children
    ([3, 0, 5, 0], 0, 8, (4, 8, -1)),                            # a prefix that fills cap exactly (the trailing 0 rides along)
    ([3, 0, 5, 1], 0, 8, (3, 8, -1)),                            # ... and the parent behind it waits
    ([3, 5, 1], 0, 8, (2, 8, -1)),
    ([3, 6, 1], 0, 8, (1, 3, -1)),                               # one over: the prefix ends before it
    ([3, 6, 1], 1, 8, (2, 7, -1)),                               # from a cursor
    ([593], 0, 593, (1, 593, -1)),                               # the largest legal position fits its own level
    ([594], 0, 593, (0, 0, 0)),                                  # one more must refuse
    ([2, 594, 1], 0, 593, (1, 2, 1)),                            # the blocking row is named as soon as the prefix ends at it
    ([2, 594, 1], 1, 593, (0, 0, 1)),
    ([4, 4], 2, 8, (0, 0, -1)),                                  # the cursor at the end: nothing left
    ([-3, 2], 0, 2, (2, 2, -1)),                                 # a negative count reads as 0
]


def so_perft(sfen: str, depth: int, max_ply: int = 500) -> int:
    """The oracle's move-generation perft of a position."""
    env = OracleVecEnv(1, max_ply)
    env.reset()
    env.set_state(0, *parse_sfen(sfen))
    return env.perft(depth)


def oracle_env_perft(sfen: str, depth: int, max_ply: int = 500) -> np.ndarray:
    """Perft under the env's game rules on ``OracleVecEnv(1, max_ply)``: ``by_depth`` (depth, 4) uint64 with the columns of
    ``PerftResult`` -- nodes, ended by checkmate, ended otherwise, side to move in check.  Every node replays its path from
    the root (``set_state``, then one ``step`` per move), so ply and history are the env's; a node whose game ended has no
    successors, and its check column is read from the restarted game, as on the device."""
    board, hands, side = parse_sfen(sfen)
    env = OracleVecEnv(1, max_ply)
    env.reset()
    by_depth = np.zeros((depth, 4), np.uint64)

    def replay(path):
        env.set_state(0, board, hands, side)
        out = None
        for a in path:
            out = env.step(np.array([a], np.int64))
        return out

    def walk(path, legal):
        k = len(path)
        for a in np.flatnonzero(legal):
            out = replay(path + [int(a)])
            ended = bool(out["terminated"][0] or out["truncated"][0])
            mate = ended and int(out["termination_reason"][0]) == S.R_CHECKMATE
            *_, mover, _ = env.state(0)
            by_depth[k] += np.array([1, mate, ended and not mate, env.in_check(0, mover)], np.uint64)
            if not ended and k + 1 < depth:
                walk(path + [int(a)], out["legal_masks"][0])

    env.set_state(0, board, hands, side)
    walk([], env.observe(0)[1])
    return by_depth


@lru_cache(maxsize=None)
def env_perft(sfen: str, depth: int, max_ply: int = 500) -> np.ndarray:
    """``oracle_env_perft``, computed once per argument and shared; treat the array as read-only."""
    out = oracle_env_perft(sfen, depth, max_ply)
    out.setflags(write=False)
    return out
