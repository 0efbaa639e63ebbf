"""Shared by tests/test_mate3_cpu.py, tests/test_hip_mate3_search.py and tests/test_hip_mate3_arena.py: the expectation of
the mate in three from the C oracle alone, on top of ``mate_search_helpers.oracle_checks``, and six hand-built positions.

The expectation (``expected3``) restates the definition of csrc/mate3.hip on a scratch oracle env (``set_state``, ``play``,
``state``, ``observe``): the root's checking moves cut at ``max_checks``; if none of them mates, the children's evasion
counts, the budget walk over ``evasion_rows`` grandchild rows, a mate in one cut at ``reply_checks`` at every grandchild,
the proving set and the choice.  The scratch env has no history, so a child or grandchild is "open" exactly when its side
to move has a legal move; this equals the device only where no repetition and no move limit can end a line.
"""
from dataclasses import dataclass, field
from functools import lru_cache
from typing import List

import numpy as np

import mate_search_helpers as H
from mate_search_helpers import mirror_sfen
from keisei_amd.shogi_gym import parse_sfen
from oracle import shogi as S

# name -> (SFEN, why it is in the set); Black to move, the "_white" twins are the mirrored positions
POSITIONS = {
    "simple": ("7kn/9/6gB1/9/5+R3/9/9/9/4K4 b G 1", "one check of nine proves, a single forced evasion"),
    "two_ways": ("9/4+P3k/9/6S2/9/4+P4/9/9/4K4 b GS 1", "two checks prove: the lowest is played, the other stays when incoming"),
    "none": ("6k2/9/4+R4/9/9/9/9/9/4K4 b S 1", "six checks with two or three evasions each, none proves"),
    "late": ("9/7k1/9/8G/3+R1S3/9/9/9/4K4 b G 1", "38 evasions over nine checks; only the ninth proves, by the tenth reply check"),
    "interpose": ("9/9/8k/6+R2/6p2/7K1/8S/9/9 b RLPnl 1", "22 checks; the defender drops from hand against the distant ones"),
    "pawn_drop3": ("9/8k/6+R1n/9/9/4+P4/9/9/4K4 b P 1", "the only third-ply mate is a pawn drop: absent from the mask, so none"),
}
for _name in list(POSITIONS):
    POSITIONS[_name + "_white"] = (mirror_sfen(POSITIONS[_name][0]), "White to move: " + POSITIONS[_name][1])
NAMES = tuple(POSITIONS)
PROVING = ("simple", "two_ways", "late", "interpose")
# the arena's start pool: the positions whose mate in three 16 checks, 64 rows and 16 reply checks find (interpose has 22
# checks and needs 75 rows), for both colours; max_checks 16 then finds the mate in one behind every reply
POOL_CAPS = (16, 64, 16)
POOL = tuple(n + s for n in ("simple", "two_ways", "late") for s in ("", "_white"))


def position(name: str):
    """``(board uint8[81], hands uint8[2, 7], side)`` of a named position."""
    return parse_sfen(POSITIONS[name][0])


def pool_sfens():
    return [POSITIONS[n][0] for n in POOL]


@dataclass
class Expected3:
    checks: List[int]                  # the root's checking moves, uncapped
    forked: List[int]                  # the first max_checks of them
    truncated: bool                    # cut 1: more checking moves than were forked
    mate1: int                         # the lowest mate in one among the forked, -1
    active: bool = False               # active at depth three
    n: List[int] = field(default_factory=list)          # per forked slot: evasions of the (open) child, -1 = not open
    first: List[int] = field(default_factory=list)      # per forked slot: its first grandchild row, -1 = without rows
    rows: int = 0                      # grandchild rows used
    reply_rows: int = 0                # third-ply rows used
    skipped: int = 0                   # cut 2: open children the budget left without rows
    reply_truncated: bool = False      # cut 3: a refuting grandchild had more checking moves than were forked
    proving: List[int] = field(default_factory=list)    # the slots that prove

    @property
    def mate3(self) -> int:
        """The lowest proving check, -1."""
        return self.forked[self.proving[0]] if self.proving else -1

    @property
    def cut(self) -> bool:
        return self.truncated or self.skipped > 0 or self.reply_truncated

    def choice(self, incoming: int) -> int:
        """What ``actions[e]`` holds after the stage."""
        if self.mate1 >= 0 or not self.proving:
            return incoming if self.mate1 < 0 else self.mate1
        return incoming if incoming in [self.forked[j] for j in self.proving] else self.mate3


def _after(board, hands, side, action):
    """The position after a legal action, by the oracle: ``(board, hands, side, legal mask)``."""
    env = H._scratch()
    frm, to, promote, drop = S.decode(int(action), white=bool(side))
    env.set_state(0, np.asarray(board, np.uint8).reshape(81), np.asarray(hands, np.uint8).reshape(14), int(side))
    env.play(0, frm, to, bool(promote), drop)
    b, h, s, _ = env.state(0)
    _, legal = env.observe(0)
    return b.copy(), h.copy(), s, legal


def expected3(board, hands, side, max_checks: int, evasion_rows: int, reply_checks: int, rows_per_env=None) -> Expected3:
    """Steps 1-7 of the definition.  ``rows_per_env``: the launch's G when it is below ``evasion_rows``."""
    checks, mates, _ = H.oracle_checks(board, hands, side)
    forked, truncated, mate1 = H.expected_record(checks, mates, max_checks)
    x = Expected3(list(checks), forked, truncated, mate1)
    if not forked or mate1 >= 0 or evasion_rows <= 0:
        return x
    x.active = True
    left = evasion_rows if rows_per_env is None else min(evasion_rows, rows_per_env)
    children = []
    for c in forked:                                           # 1, 2: no forked check mates, so every child has a reply
        child = _after(board, hands, side, c)
        n = int(child[3].sum())
        assert n >= 1
        children.append(child)
        x.n.append(n)
        if n <= left:                                          # 3: the budget walk
            x.first.append(x.rows)
            x.rows += n
            left -= n
        else:
            x.first.append(-1)
            x.skipped += 1
    for j, child in enumerate(children):
        if x.first[j] < 0:
            continue
        proves = True
        for ev in np.flatnonzero(child[3]):                    # 4: the grandchildren, ascending in action
            gb, gh, gs, glegal = _after(child[0], child[1], child[2], ev)
            if not glegal.any():                               # the evasion mates the attacker: not open, refutes
                proves = False
                continue
            checks3, mates3, _ = H.oracle_checks(gb, gh, gs)   # 5: mate in one, cut at reply_checks
            forked3, trunc3, mate = H.expected_record(checks3, mates3, reply_checks)
            x.reply_rows += len(forked3)
            if mate < 0:
                proves = False
                x.reply_truncated |= trunc3
        if proves:                                             # 6
            x.proving.append(j)
    return x


@lru_cache(maxsize=None)
def expected(name: str, max_checks: int, evasion_rows: int, reply_checks: int) -> Expected3:
    """``expected3`` of a named position, computed once and shared."""
    return expected3(*position(name), max_checks, evasion_rows, reply_checks)


def expected_words(x: Expected3, cap: int, incoming: int):
    """The device's record of csrc/mate3.hip as a list of ``6 + 2 * cap`` ints, for an env whose incoming action is
    ``incoming``."""
    from keisei_amd.training.mate_search import (FLAG3_ACTIVE, FLAG3_CHANGED, FLAG3_MATE, FLAG3_REPLY_TRUNCATED,
                                                 FLAG3_SKIPPED)
    flags, slot, action, mask = 0, -1, x.choice(incoming), 0   # (a mate in one is in actions[e] before this stage looks)
    if x.active:
        flags |= FLAG3_ACTIVE | (FLAG3_SKIPPED if x.skipped else 0) | (FLAG3_REPLY_TRUNCATED if x.reply_truncated else 0)
        for j in x.proving:
            mask |= 1 << j
        if x.proving:
            slot = x.forked.index(action)
            flags |= FLAG3_MATE | (FLAG3_CHANGED if action != incoming else 0)
    signed = lambda v: v - (1 << 32) if v >= 1 << 31 else v  # noqa: E731
    pad = [-1] * (cap - len(x.n))
    return [flags, x.rows, slot, action, signed(mask & 0xffffffff), signed(mask >> 32)] + x.n + pad + x.first + pad
