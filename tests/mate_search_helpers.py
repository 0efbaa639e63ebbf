"""Shared by tests/test_mate_search_cpu.py, tests/test_hip_mate_search.py and tests/test_hip_mate_arena.py: the expectation
of the mate-in-one check from the C oracle alone, and a dozen hand-built positions, each chosen for a way the kernel
(csrc/mate.hip) can go wrong.

The expectation (``oracle_checks``): for a position and every legal action, apply the move on a scratch oracle env
(``set_state``, then ``play``); the move gives check when ``in_check(opponent)`` holds after it and mates when the opponent
also has ``legal_count == 0``.  The scratch env has no history, so the definition equals the env step's verdict only where
neither a repetition nor the move limit can end the game with that move.
"""
from functools import lru_cache

import numpy as np

from keisei_amd.shogi_gym import format_sfen, parse_sfen
from oracle import shogi as S
from oracle.shogi import OracleVecEnv

START = "lnsgkgsnl/1r5b1/ppppppppp/9/9/9/PPPPPPPPP/1B5R1/LNSGKGSNL b - 1"


def mirror_sfen(sfen: str) -> str:
    """The same position with the colours swapped and the board turned: what was Black's to move is White's."""
    board, hands, side = parse_sfen(sfen)
    turned = board[::-1].copy()
    turned[turned != 0] ^= S.WHITE
    return format_sfen(turned, hands[::-1], side ^ 1)


# name -> (SFEN, why it is in the set)
POSITIONS = {
    "start": (START, "no checking move at all"),
    "gold_head": ("4k4/9/4PG3/9/9/9/9/9/4K4 b - 1", "a gold on the head: a mate by a board move"),
    "gold_drop": ("4k4/9/4P4/9/9/9/9/9/4K4 b G 1", "a mate by a non-pawn drop"),
    "pawn_drop": ("7nk/9/8G/9/9/9/9/9/4K4 b P 1", "the only mate would be a pawn drop: absent from the mask, so none"),
    "discovered": ("8k/6G2/8B/9/9/9/9/9/4K3R b - 1", "the bishop steps off the rook's file: it does not attack the king itself"),
    "double": ("4k4/2G6/4BP3/9/4R4/9/9/9/4K4 b - 1", "a double check: the bishop checks and uncovers the rook"),
    "promote": ("7lk/9/4R4/9/9/9/9/9/4K4 b - 1", "R-1c mates only as a dragon; the plain rook move is legal and checks too"),
    "knight": ("7sk/7bl/9/9/6N2/9/9/9/4K4 b - 1", "a smothered king: a knight jump mates"),
    "capture": ("4k4/4p4/4PG3/9/9/9/9/9/4K4 b - 1", "a mate by capture"),
    "evasion": ("4k4/4g4/4KG3/9/9/9/9/9/9 b - 1", "the mover is in check; one evasion, the capture of the checker, mates"),
    "open": ("4K4/9/9/9/9/9/5B3/9/8k b RBGL 1", "more than 16 checking moves over the whole mask row; the only mate, G*2i, is late in action order"),
}
POSITIONS["gold_drop_white"] = (mirror_sfen(POSITIONS["gold_drop"][0]), "White to move: a drop, seen from the other side")
POSITIONS["knight_white"] = (mirror_sfen(POSITIONS["knight"][0]), "White to move: a knight jump, seen from the other side")
NAMES = tuple(POSITIONS)
WITH_MATE = ("gold_head", "gold_drop", "discovered", "double", "promote", "knight", "capture", "gold_drop_white",
             "knight_white", "evasion")
WITHOUT_MATE = ("start", "pawn_drop")
# the arena's start pool: the mate-in-one positions whose mover is not in check, for both colours
POOL = ("gold_head", "gold_drop", "discovered", "double", "promote", "knight", "capture")


def position(name: str):
    """``(board uint8[81], hands uint8[2, 7], side)`` of a named position."""
    return parse_sfen(POSITIONS[name][0])


def pool_sfens():
    return [f(POSITIONS[n][0]) for n in POOL for f in (lambda s: s, mirror_sfen)]


_SCRATCH = {}


def _scratch() -> OracleVecEnv:
    if "env" not in _SCRATCH:
        _SCRATCH["env"] = OracleVecEnv(1, 500)
        _SCRATCH["env"].reset()
    return _SCRATCH["env"]


def oracle_checks(board, hands, side: int):
    """``(checks, mates, legal)`` of a position by the oracle alone: the legal actions that give check and the ones that
    mate, ascending, and the bool legal mask."""
    env = _scratch()
    board, hands, side = np.asarray(board, np.uint8).reshape(81), np.asarray(hands, np.uint8).reshape(14), int(side)
    env.set_state(0, board, hands, side)
    _, legal = env.observe(0)
    checks, mates = [], []
    for a in np.flatnonzero(legal):
        frm, to, promote, drop = S.decode(int(a), white=bool(side))
        env.set_state(0, board, hands, side)
        env.play(0, frm, to, bool(promote), drop)
        if env.in_check(0, side ^ 1):
            checks.append(int(a))
            if env.legal_count(0) == 0:
                mates.append(int(a))
    return checks, mates, legal


@lru_cache(maxsize=None)
def expected(name: str):
    """``oracle_checks`` of a named position, computed once and shared: ``(checks, mates)`` as tuples."""
    checks, mates, _ = oracle_checks(*position(name))
    return tuple(checks), tuple(mates)


# Two scripted lines from the start position, as (from, to) squares (row, column; row 0 is White's back rank), that end
# with a bishop's capture with check on the board: 1. P-7f 2. P-8d 3. P-2f 4. P-8e 5. P-2e and a quiet sixth move (Black's
# bishop takes 3c with check, ply 6), and 1. P-2f 2. P-3d 3. P-2e 4. P-9d and a quiet fifth move (White's bishop takes 7g
# with check, ply 5).  The last move differs per env, so the envs' rows differ.
LINES = {
    "even": ([((6, 2), (5, 2)), ((2, 1), (3, 1)), ((6, 7), (5, 7)), ((3, 1), (4, 1)), ((5, 7), (4, 7))],
             [((2, 0), (3, 0)), ((2, 8), (3, 8)), ((2, 2), (3, 2)), ((2, 3), (3, 3)), ((2, 4), (3, 4))]),
    "odd": ([((6, 7), (5, 7)), ((2, 6), (3, 6)), ((5, 7), (4, 7)), ((2, 0), (3, 0))],
            [((6, 8), (5, 8)), ((6, 0), (5, 0)), ((6, 6), (5, 6)), ((6, 5), (5, 5)), ((6, 4), (5, 4))]),
}


@lru_cache(maxsize=None)
def line(which: str):
    """``(actions (plies, envs) int64, expect)`` of a scripted line, played on the oracle in lockstep (every move is legal
    by its mask): ``expect`` is per env ``(checks, mates)`` of ``oracle_checks`` at the end, where every env stands at ply
    ``plies``."""
    common, last = LINES[which]
    n = len(last)
    ref = OracleVecEnv(n, 500)
    _, mask = ref.reset()
    acts = []
    for k in range(len(common) + 1):
        moves = [common[k]] * n if k < len(common) else last
        a = np.array([S.encode(S.sq(*f), S.sq(*t), white=bool(k & 1)) for f, t in moves], np.int64)
        assert all(mask[i][a[i]] for i in range(n)), (which, k, a)
        mask = ref.step(a)["legal_masks"]
        acts.append(a)
    ends = [ref.state(i) for i in range(n)]
    assert all(ply == len(acts) for *_, ply in ends)
    return np.stack(acts), [oracle_checks(b, h, s)[:2] for b, h, s, _ in ends]


def expected_record(checks, mates, cap: int):
    """What a cap allows: ``(forked list, truncated, mate action or -1)`` -- the first ``cap`` checking moves, whether more
    exist, and the lowest mate among the forked ones."""
    forked = list(checks[:cap])
    hit = [a for a in forked if a in set(mates)]
    return forked, len(checks) > cap, (hit[0] if hit else -1)
