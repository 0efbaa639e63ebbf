"""GameFeatureTracker: per-game style features taken from the actions and the step metadata of match play (the
reference's keisei/training/game_feature_tracker.py; same public names, arguments and rows).

Everything is read off the spatial action index (square * 139 + move type, in the mover's perspective) and the env's
StepMetadata; no game is replayed.  Two paths end in the same rows:

* the CPU path, ``record_step`` once per ply over host arrays, as the reference's ``play_batch`` drives it;
* the device path of ``MatchArena(features=True)``: ``ka_arena_features_step`` (csrc/arena.hip) keeps the same per-env
  accumulators in HBM and writes one *game record* per finished game; ``GameFeatureTracker.from_records`` expands the
  records into rows.

The CPU path goes through the same records (``tracker.records``), so a record is the one place where a finished game
becomes its two rows.  Record layout, ``RECORD_WORDS`` int32 (csrc/arena.hip, ``ka_arena_feature_words(1)``):

    0 env index   1 total plies   2 termination reason   3 last mover   4 reward sign (-1, 0, 1)
    5 opening actions kept (0..12)   6 num_repetitions   7 ply of the round / step of the tracker
    8..19 the opening actions   20..29 side A   30..39 side B, each in ``SIDE_FIELDS`` order with -1 for None
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np

# spatial action encoding (spatial_action_mapper.rs): 139 move types per square
SPATIAL_MOVE_TYPES = 139
PROMOTION_MOVE_TYPE_MIN = 64            # 64..131: sliding and knight moves with promotion
PROMOTION_MOVE_TYPE_MAX = 131
DROP_MOVE_TYPE_MIN = 132                # 132..138: drops of the seven hand piece types
DROP_MOVE_TYPE_MAX = 138
NO_CAPTURE = 255                        # StepMetadata.captured_piece when nothing was taken

# Source squares are in the mover's perspective (rotated for white), so black's home squares serve both sides.
BLACK_ROOK_SQUARE = 79                  # row 8, col 7
BLACK_KING_SQUARE = 76                  # row 8, col 4

EARLY_DROP_PLY_THRESHOLD = 40
OPENING_SEQ_3_LEN = 3
OPENING_SEQ_6_LEN = 6
ROOK_MOBILITY_PLY = 20
KING_MOVEMENT_PLY = 30
_KING_DISPLACEMENT_PLY = 20
_OPENING_KEPT = 2 * OPENING_SEQ_6_LEN   # actions kept since the accumulator's reset, both sides interleaved

SIDE_FIELDS = ("first_capture_ply", "first_drop_ply", "num_captures", "num_drops", "num_promotions", "num_early_drops",
               "rook_moved_ply", "rook_moves_in_20", "king_displacement_20", "king_moves_in_30")
_OPTIONAL = ("first_capture_ply", "first_drop_ply", "rook_moved_ply")
_REC_HEAD = 8
_REC_SIDE = _REC_HEAD + _OPENING_KEPT
RECORD_WORDS = _REC_SIDE + 2 * len(SIDE_FIELDS)
ACC_WORDS = 2 + _OPENING_KEPT + 2 * len(SIDE_FIELDS)     # {actions kept, num_repetitions}, the actions, the two sides


def classify_action(action_id: int) -> Tuple[bool, bool, int]:
    """``(is_drop, is_promotion, square)`` of a spatial action: the source square of a board move, the destination of a
    drop, both in the mover's perspective."""
    square, move_type = divmod(action_id, SPATIAL_MOVE_TYPES)
    return (DROP_MOVE_TYPE_MIN <= move_type <= DROP_MOVE_TYPE_MAX,
            PROMOTION_MOVE_TYPE_MIN <= move_type <= PROMOTION_MOVE_TYPE_MAX, square)


@dataclass
class _SideStats:
    first_capture_ply: Optional[int] = None
    first_drop_ply: Optional[int] = None
    num_captures: int = 0
    num_drops: int = 0
    num_promotions: int = 0
    num_early_drops: int = 0
    rook_moved_ply: Optional[int] = None
    rook_moves_in_20: int = 0
    king_displacement_20: int = 0
    king_moves_in_30: int = 0

    def reset(self) -> None:
        self.__init__()

    def words(self) -> List[int]:
        return [-1 if getattr(self, k) is None else int(getattr(self, k)) for k in SIDE_FIELDS]


@dataclass
class GameFeatureAccumulator:
    """One env's running game: ``sides[0]`` is player A (black), ``sides[1]`` player B (white); the opening actions and
    the repetition count belong to the game."""

    actions: List[int] = field(default_factory=list)
    sides: List[_SideStats] = field(default_factory=lambda: [_SideStats(), _SideStats()])
    num_repetitions: int = 0
    _ply: int = 0

    def reset(self) -> None:
        self.actions.clear()
        for s in self.sides:
            s.reset()
        self.num_repetitions = 0
        self._ply = 0

    def words(self) -> List[int]:
        """The accumulator as the device keeps it (``ACC_WORDS`` int32, ``ka_arena_feature_words(0)``)."""
        kept = list(self.actions) + [0] * (_OPENING_KEPT - len(self.actions))
        return [len(self.actions), self.num_repetitions] + kept + self.sides[0].words() + self.sides[1].words()


@dataclass
class GameFeatureRow:
    """One side of one finished game, as the ``game_features`` table takes it."""

    checkpoint_id: int
    opponent_id: int
    epoch: int
    side: str                            # "black" | "white"
    result: str                          # "win" | "loss" | "draw"
    total_plies: int
    first_action: Optional[int]
    opening_seq_3: Optional[str]
    opening_seq_6: Optional[str]
    rook_moved_ply: Optional[int]
    king_displacement_20: int
    first_capture_ply: Optional[int]
    first_drop_ply: Optional[int]
    num_captures: int
    num_drops: int
    num_promotions: int
    num_early_drops: int
    rook_moves_in_20: int
    king_moves_in_30: int
    num_repetitions: int
    termination_reason: int

    def to_dict(self) -> Dict[str, Any]:
        """The argument of ``write_game_features()``: the 21 columns in the table's order."""
        return {k: getattr(self, k) for k in self.__dataclass_fields__}


def _opening(actions: Sequence[int], length: int) -> Optional[str]:
    return ",".join(str(a) for a in actions[:length]) if len(actions) >= length else None


def _rows_of_record(rec: Sequence[int], entry_a_id: int, entry_b_id: int, epoch: int) -> List[GameFeatureRow]:
    """A game record as its black row and its white row."""
    rec = [int(v) for v in rec]
    _, total_plies, reason, last_mover, sign, kept, repetitions = rec[:7]
    winner = last_mover if sign > 0 else 1 - last_mover if sign < 0 else -1
    opening = rec[_REC_HEAD:_REC_HEAD + kept]
    rows = []
    for idx, name in ((0, "black"), (1, "white")):
        mine = opening[idx::2]                               # the list alternates A, B, A, ... from the reset on
        side = dict(zip(SIDE_FIELDS, rec[_REC_SIDE + idx * len(SIDE_FIELDS):_REC_SIDE + (idx + 1) * len(SIDE_FIELDS)]))
        for k in _OPTIONAL:
            if side[k] < 0:
                side[k] = None
        rows.append(GameFeatureRow(
            checkpoint_id=entry_b_id if idx else entry_a_id, opponent_id=entry_a_id if idx else entry_b_id, epoch=epoch,
            side=name, result="win" if winner == idx else "draw" if winner == -1 else "loss", total_plies=total_plies,
            first_action=mine[0] if mine else None, opening_seq_3=_opening(mine, OPENING_SEQ_3_LEN),
            opening_seq_6=_opening(mine, OPENING_SEQ_6_LEN), num_repetitions=repetitions, termination_reason=reason,
            **side))
    return rows


class GameFeatureTracker:
    """Features of the games of one pairing over ``num_envs`` envs::

        tracker = GameFeatureTracker(num_envs, entry_a_id, entry_b_id, epoch)
        tracker.record_step(actions, captured_piece, termination_reason, ply_count, pre_step_players,
                            terminated, truncated, rewards)          # once per ply
        rows = tracker.completed_rows                                # two per finished game, black first

    ``records`` holds the finished games as (games, RECORD_WORDS) int32 for bulk insertion."""

    def __init__(self, num_envs: int, entry_a_id: int, entry_b_id: int, epoch: int) -> None:
        self.num_envs = num_envs
        self.entry_a_id = entry_a_id                         # player A = side 0 (black)
        self.entry_b_id = entry_b_id                         # player B = side 1 (white)
        self.epoch = epoch
        self.accumulators = [GameFeatureAccumulator() for _ in range(num_envs)]
        self.completed_rows: List[GameFeatureRow] = []
        self._records: List[Sequence[int]] = []
        self._steps = 0

    @classmethod
    def from_records(cls, records, entry_a_id: int, entry_b_id: int, epoch: int, num_envs: int = 0) -> "GameFeatureTracker":
        """The device path: ``records`` is (games, RECORD_WORDS) int32 as ``ka_arena_features_step`` wrote it, in the
        order the games finished."""
        records = np.asarray(records, dtype=np.int32).reshape(-1, RECORD_WORDS)
        self = cls(num_envs, entry_a_id, entry_b_id, epoch)
        for rec in records:
            self._records.append(rec)
            self.completed_rows += _rows_of_record(rec, entry_a_id, entry_b_id, epoch)
        return self

    @property
    def records(self) -> np.ndarray:
        return np.asarray(self._records, dtype=np.int32).reshape(-1, RECORD_WORDS)

    def record_step(self, actions: np.ndarray, captured_piece: np.ndarray, termination_reason: np.ndarray,
                    ply_count: np.ndarray, pre_step_players: np.ndarray, terminated: np.ndarray, truncated: np.ndarray,
                    rewards: np.ndarray) -> None:
        """One step of all envs.  ``pre_step_players``: who moved (0 = A, 1 = B); ``rewards`` are the mover's;
        ``ply_count`` is the env's count after the move, for a finished game that game's length."""
        done = np.asarray(terminated, dtype=bool) | np.asarray(truncated, dtype=bool)
        for i in range(self.num_envs):
            acc = self.accumulators[i]
            action, ply, mover = int(actions[i]), int(ply_count[i]), int(pre_step_players[i])
            acc._ply = ply
            side = acc.sides[mover]
            is_drop, is_promotion, square = classify_action(action)
            if len(acc.actions) < _OPENING_KEPT:             # the first 12 actions since the reset, whatever their ply
                acc.actions.append(action)
            if int(captured_piece[i]) != NO_CAPTURE:
                side.num_captures += 1
                if side.first_capture_ply is None:
                    side.first_capture_ply = ply
            if is_drop:
                side.num_drops += 1
                if side.first_drop_ply is None:
                    side.first_drop_ply = ply
                if ply <= EARLY_DROP_PLY_THRESHOLD:
                    side.num_early_drops += 1
            if is_promotion:
                side.num_promotions += 1
            if not is_drop and square == BLACK_ROOK_SQUARE:
                if side.rook_moved_ply is None:
                    side.rook_moved_ply = ply
                if ply <= ROOK_MOBILITY_PLY:
                    side.rook_moves_in_20 += 1
            if not is_drop and square == BLACK_KING_SQUARE:
                if ply <= _KING_DISPLACEMENT_PLY:
                    side.king_displacement_20 += 1
                if ply <= KING_MOVEMENT_PLY:
                    side.king_moves_in_30 += 1
            if done[i]:
                reason = int(termination_reason[i])
                if reason == 2:                              # repetition is counted where it ends the game, nowhere else
                    acc.num_repetitions += 1
                self._emit_game(i, ply, reason, mover, float(rewards[i]))
        self._steps += 1

    def _emit_game(self, env_idx: int, total_plies: int, termination_reason: int, last_mover: int, reward: float) -> None:
        acc = self.accumulators[env_idx]
        sign = 1 if reward > 0 else -1 if reward < 0 else 0   # a NaN is a draw
        rec = [env_idx, total_plies, termination_reason, last_mover, sign] + acc.words()[:2] + [self._steps] + acc.words()[2:]
        self._records.append(rec)
        self.completed_rows += _rows_of_record(rec, self.entry_a_id, self.entry_b_id, self.epoch)
        acc.reset()                                          # the VecEnv has restarted the game
