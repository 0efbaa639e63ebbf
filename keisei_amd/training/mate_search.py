"""Mate in one for the device ply, per model.

The sampler, the lookahead and the tree search judge a move through the value head; a mate in one that is not among the
first moves by raw logit is walked past.  Here the rules answer: ``ka_mate_fork`` (csrc/mate.hip) finds the legal moves that
give check -- the set bits of the env's packed mask, each laid over the board in LDS and the other king tested by looking
outward from it -- and copies one child row per checking move; the env's own ``ka_shogi_env_step`` steps the child rows; and
``ka_mate_choose`` replaces the action of an env that has a child ended by checkmate in the mover's favour.  No forward runs.
The reference has nothing like it: it never searches.

Semantics.  Row ``m`` of the controls table belongs to model ``m``: ``max_checks`` (0..64, 0 = the model's action stands) and
``skip_plies`` (a position whose game ply is below it is left alone).  A row outside these ranges reads as off; ``max_checks``
above the launch's ``cap`` is cut to it.  Env ``e`` with model ``m = model_of[e]`` is *active* when ``m`` lies in ``[0, K)``,
the row is on, its game ply is ``>= skip_plies_m`` and it has a checking move.  The *checking moves* are taken in ascending
action order and the first ``min(max_checks_m, cap)`` are forked; more than that sets the record's *truncated* bit.  A child is
a *mate* when the env step terminated it by checkmate with a positive reward for the mover -- the step's verdict is the
definition, so a checking move that ends the game by repetition, perpetual check or the move limit is not one.  An incoming
action that is itself a mate stays; otherwise the mate with the lowest action index is played; an env without a mate keeps
its action, and nothing else about the ply changes.

Mate in three (``Mate3Search``, csrc/mate3.hip) stands behind it for the models whose row has ``evasion_rows`` > 0.  An env
that is active above and has no mate in one is *active at depth three*.  A child the step neither terminated nor truncated
is *open*; its evasions are the set bits of its new mask.  A budget of ``min(evasion_rows, G)`` grandchild rows is walked
over the children in slot order: an open child whose evasions fit gets one row per evasion, ascending; one whose evasions do
not fit is skipped and the walk goes on.  The env step steps the grandchild rows; one that it terminated or truncated
refutes its check.  The three stages above then run with the grandchild rows as their envs and ``reply_checks`` as their
``max_checks``.  A child *proves* when it got rows and every grandchild of it is open and has a mate in one; a proving
incoming action stays, otherwise the proving check with the lowest action is played.  Caps and the budget only ever turn a
mate into "not proven"; the records say when one cut.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import ClassVar, Optional, Tuple

import numpy as np
import torch

from keisei_amd import _lib
from keisei_amd.shogi_gym import ACTION_SPACE, MASK_WORDS

from ._forked_rows import ForkedRows, PlyStage, check_int, check_search_env, controls_rows

__all__ = ["MateControls", "MateStats", "MateSearch", "mate_table", "mate_words", "arena_mate", "MAX_CHECKS",
           "MAX_SKIP_PLIES", "MAX_EVASION_ROWS", "Mate3Stats", "Mate3Search", "mate3_words", "mate3_reply_table",
           "arena_mate3"]

MAX_CHECKS = 64
MAX_SKIP_PLIES = 65535
MAX_EVASION_ROWS = 128
# record words (csrc/mate.hip; ka_mate_words reports the sizes)
REC_FLAGS, REC_NCHECKS, REC_SLOT, REC_ACTION, REC_LIST = 0, 1, 2, 3, 4
FLAG_ACTIVE, FLAG_MATE, FLAG_CHANGED, FLAG_TRUNCATED = 1, 2, 4, 8
ERR_CHILD_STEP = 2
# the record of the mate in three (csrc/mate3.hip; ka_mate3_words reports the sizes): the n_i follow at REC3_N, the slots'
# first rows behind them
REC3_FLAGS, REC3_ROWS, REC3_SLOT, REC3_ACTION, REC3_PROVING, REC3_N = 0, 1, 2, 3, 4, 6
FLAG3_ACTIVE, FLAG3_MATE, FLAG3_CHANGED, FLAG3_SKIPPED, FLAG3_REPLY_TRUNCATED = 1, 2, 4, 8, 16
ERR3_CHILD_STEP, ERR3_GRAND_STEP, ERR3_THIRD_STEP = 2, 4, 8


def mate_words(cap: int) -> int:
    """32-bit words of one record."""
    return REC_LIST + int(cap)


@dataclass(frozen=True)
class MateControls:
    """One model's mate controls.  ``max_checks`` 0 is off.  ``evasion_rows`` > 0 (with ``reply_checks`` > 0) adds the mate
    in three behind the mate in one: the budget of grandchild rows per position, one per evasion of a check, and the
    checking moves tried at the third ply."""
    max_checks: int = 16
    skip_plies: int = 0
    evasion_rows: int = 0
    reply_checks: int = 0

    OFF: ClassVar["MateControls"]

    def __post_init__(self) -> None:
        for name, hi in (("max_checks", MAX_CHECKS), ("skip_plies", MAX_SKIP_PLIES), ("evasion_rows", MAX_EVASION_ROWS),
                         ("reply_checks", MAX_CHECKS)):
            object.__setattr__(self, name, check_int(name, getattr(self, name), 0, hi))
        if (self.evasion_rows > 0) != (self.reply_checks > 0):
            raise ValueError(f"evasion_rows and reply_checks must be both zero or both positive, got {self.evasion_rows} "
                             f"and {self.reply_checks}")

    def row(self) -> np.ndarray:
        """The table row: int32 max_checks, skip_plies, evasion_rows, reply_checks (csrc/mate.hip reads the first two)."""
        return np.array([self.max_checks, self.skip_plies, self.evasion_rows, self.reply_checks], dtype=np.int32)


MateControls.OFF = MateControls(0)


@dataclass
class MateStats:
    """The counters ``ka_mate_choose`` adds to."""
    positions: int = 0     # active envs (with a checking move), summed over the plies
    forked: int = 0        # child rows in use
    mates: int = 0         # positions with a mate in one
    changed: int = 0       # of these, the ones whose incoming action was not a mate already
    truncated: int = 0     # active positions with more checking moves than were forked


def _rows(controls, K: int):
    return controls_rows(controls, K, MateControls, "mate", by_index=True)


def mate_table(controls, K: int) -> np.ndarray:
    """The ``(K, 4)`` int32 table.  ``controls``: None (K rows ``OFF``), one ``MateControls`` (every model), a sequence of
    exactly K or a dict from model index to ``MateControls`` (a model not named is off)."""
    return np.stack([r.row() for r in _rows(controls, K)]).astype(np.int32, copy=False)


def arena_mate(mate, num_models: int, collect: bool) -> Tuple[Optional[np.ndarray], int]:
    """``MatchArena``'s reading of ``mate=``: None stays None (the ply is what it was); everything else is a table of
    ``num_models`` rows and the largest ``max_checks`` in it, the cap of the child rows -- refused with ``collect=True``,
    where ``DynamicTrainer`` treats the recorded actions as draws from the entry's own policy, which a mating move put in
    the place of the sampler's is not (the logged log-prob would not be the played move's)."""
    if mate is None:
        return None, 0
    if collect:
        raise ValueError("mate cannot be combined with collect=True: DynamicTrainer treats the recorded actions as draws "
                         "from the entry's own policy, and the logged log-prob would not be the played move's")
    rows = _rows(mate, num_models)
    return mate_table(rows, num_models), max(r.max_checks for r in rows)


def mate3_reply_table(table: np.ndarray) -> np.ndarray:
    """The third ply's ``(K, 4)`` table of a controls table: word 0 ``reply_checks`` of the rows with depth three on (0
    otherwise), the other words zero -- what the unchanged ``ka_mate_fork`` reads as ``max_checks`` / ``skip_plies``."""
    table = np.asarray(table, dtype=np.int32)
    out = np.zeros_like(table)
    er, rc = table[:, 2], table[:, 3]
    on = (er > 0) & (er <= MAX_EVASION_ROWS) & (rc >= 0) & (rc <= MAX_CHECKS)
    out[:, 0] = np.where(on, rc, 0)
    return out


def arena_mate3(mate, num_models: int) -> Tuple[int, int]:
    """``(G, cap3)`` of ``MatchArena``'s ``mate=``: the largest ``evasion_rows`` and ``reply_checks`` given, the grandchild
    rows per env and the third ply's rows per grandchild; ``(0, 0)`` when no model asks for depth three (or ``mate`` is
    None): the ply is then the mate in one's."""
    if mate is None:
        return 0, 0
    rows = _rows(mate, num_models)
    return max(r.evasion_rows for r in rows), max(r.reply_checks for r in rows)


def _check_cap(cap) -> int:
    return check_int("cap", cap, 1, MAX_CHECKS)


class MateSearch:
    """The child rows of a device ``VecEnv`` and the three stages of the mate check.  Everything is allocated here, once:
    ``cap`` child rows per env, each a state row, a key / check history row, two packed mask rows and the step's outputs
    (the rows the lookahead holds per child, minus the forward workspace: no forward runs here).  ``records()``
    (envs, 4 + cap) int32 are the envs' records of the last ``step``."""

    def __init__(self, env, cap: int) -> None:
        """``env``: the device ``VecEnv``, or the ``ForkedRows`` whose rows are this search's positions (the third ply of
        the mate in three)."""
        cap = _check_cap(cap)
        check_search_env(env.env if isinstance(env, ForkedRows) else env, None, "the mate search")
        self._child = c = ForkedRows(env, cap)
        c.alias(self, "child")                             # child_state .. child_reason, _child_err
        self.env, self.cap, self.M = c.env, cap, c.M
        self.words = _lib.query("ka_mate_words", 0, cap)
        assert self.words == mate_words(cap) and cap <= _lib.query("ka_mate_words", 3, 0) == MAX_CHECKS
        with torch.cuda.device(c.env.device):
            self._records = torch.zeros(c.parents, self.words, dtype=torch.int32, device=c.env.device)
            self._counters = torch.zeros(_lib.query("ka_mate_words", 2, cap), dtype=torch.int32, device=c.env.device)
            self._counters_host = torch.zeros(self._counters.shape, dtype=torch.int32).pin_memory()       # stats, then the error word
        self._nstats = self._counters.shape[0] - 1

    def clear(self) -> None:
        """Zero the counters, the error word and the refusal latch of the child step (a round's start)."""
        self._counters.zero_()
        self._child.clear()

    def fork(self, mask_bits, actions, model_of, table, stream) -> None:
        c = self._child
        _lib.call("ka_mate_fork", mask_bits, MASK_WORDS, actions, model_of, int(table.shape[0]), table, c.parent_state,
                  c.parent_keys, c.parent_checks, self.env._max_ply, self.cap, self._records, c.state, c.keys, c.checks,
                  c.bits_in, c.actions, c.parents, ACTION_SPACE, stream)

    def step_children(self, stream) -> None:
        self._child.step(stream)

    def choose(self, actions, stream) -> None:
        c = self._child
        _lib.call("ka_mate_choose", self._records, self.cap, c.rewards, c.terminated, c.reason, c.err, actions,
                  self._counters, self._counters.data_ptr() + 4 * self._nstats, c.parents, stream)

    def step(self, mask_bits, actions, model_of, table, stream) -> None:
        """The three stages on the current stream (``stream``: its pointer), after the sampler (and the lookahead or the
        search) and before ``env.step``: ``actions`` (envs,) int64 is overwritten where a mate replaces it.  ``mask_bits``
        the env's current packed masks, ``model_of`` (envs,) int32, ``table`` the (K, 4) int32 controls table on the
        device."""
        self.fork(mask_bits, actions, model_of, table, stream)
        self.step_children(stream)
        self.choose(actions, stream)

    def read(self) -> MateStats:
        """At a sync point: the counters since ``clear()`` (one small device -> host copy).  Raises on the error word."""
        self._counters_host.copy_(self._counters)
        c = self._counters_host.numpy()
        if int(c[self._nstats]) & ERR_CHILD_STEP:
            w = self._child_err
            raise RuntimeError(f"the mate search's child step refused an action (word "
                               f"{int(w[1].item()) or int(w[0].item()):#x}): a forked row does not match the mask it "
                               "was forked with")
        return MateStats(int(c[0]), int(c[1]), int(c[2]), int(c[3]), int(c[4]))

    def records(self) -> torch.Tensor:
        """The per-env records of the last ``step`` (a copy on the device)."""
        return self._records.clone()


def mate3_words(cap: int) -> int:
    """32-bit words of one mate-in-three record."""
    return REC3_N + 2 * int(cap)


@dataclass
class Mate3Stats:
    """The counters ``ka_mate3_choose`` adds to."""
    positions: int = 0     # envs active at depth three (checking moves, no mate in one), summed over the plies
    rows: int = 0          # grandchild rows in use: the evasions stepped
    reply_rows: int = 0    # third-ply rows in use: the checking moves stepped behind the evasions
    mates: int = 0         # positions with a mate in three
    changed: int = 0       # of these, the ones whose incoming action did not prove already
    skipped: int = 0       # open children the budget walk left without rows


class Mate3Search:
    """The mate in three of a device ``VecEnv``: a ``MateSearch`` for the root (``cap`` child rows per env), ``rows``
    grandchild rows per env -- one per evasion of the checks the budget walk takes -- and a third-ply ``MateSearch`` over
    the grandchild rows (``reply_cap`` rows each).  Everything is allocated here, once.  ``step`` runs the root's three
    stages as they are and, behind them, ``ka_mate3_fork``, the env step over the grandchild rows, ``ka_mate3_gate``, the
    third ply's three stages and ``ka_mate3_choose`` (csrc/mate3.hip)."""

    def __init__(self, env, cap: int, rows: int, reply_cap: int) -> None:
        rows = check_int("rows", rows, 1, MAX_EVASION_ROWS)
        self.root = MateSearch(env, cap)
        self.env, self.cap, self.rows, self.reply_cap = env, self.root.cap, rows, _check_cap(reply_cap)
        n, dev = env.num_envs, env.device
        self.words = _lib.query("ka_mate3_words", 0, self.cap)
        assert self.words == mate3_words(self.cap) and _lib.query("ka_mate3_words", 3, 0) == MAX_EVASION_ROWS
        # the grandchild rows lie beneath the env, `rows` per env: which child a row continues is the fork's choice
        self._grand = g = ForkedRows(env, self.rows)
        g.alias(self, "grand")                             # grand_state .. grand_reason, _grand_err
        self.M = M = g.M
        with torch.cuda.device(dev):
            z = lambda *shape, dtype: torch.zeros(*shape, dtype=dtype, device=dev)  # noqa: E731
            self._records = z(n, self.words, dtype=torch.int32)
            self.grand_model_of = z(M, dtype=torch.int32)
            self.grand_filler = z(M, dtype=torch.int64)                    # the third ply's action array: a scratch one
            self._counters = z(_lib.query("ka_mate3_words", 2, self.cap), dtype=torch.int32)      # stats, then the error word
            self._counters_host = torch.zeros(self._counters.shape, dtype=torch.int32).pin_memory()
        self.third = MateSearch(g, self.reply_cap)
        self._nstats = self._counters.shape[0] - 1

    def clear(self) -> None:
        """Zero the counters, the error words and the refusal latches of the three child steps (a round's start)."""
        self.root.clear()
        self.third.clear()
        self._counters.zero_()
        self._grand.clear()

    def fork(self, mask_bits, actions, model_of, table, stream) -> None:
        env, root, g = self.env, self.root, self._grand
        _lib.call("ka_mate3_fork", mask_bits, MASK_WORDS, actions, model_of, int(table.shape[0]), table, env._state,
                  root._records, self.cap, root.child_state, root.child_keys, root.child_checks, root.child_mask_bits,
                  root.child_terminated, root.child_truncated, env._max_ply, self.rows, self._records, g.state, g.keys,
                  g.checks, g.bits_in, g.actions, env.num_envs, ACTION_SPACE, stream)

    def step_grandchildren(self, stream) -> None:
        self._grand.step(stream)

    def gate(self, model_of, stream) -> None:
        _lib.call("ka_mate3_gate", self._records, self.cap, self.rows, model_of, self.grand_mask_bits, MASK_WORDS,
                  self.grand_terminated, self.grand_truncated, self.grand_model_of, self.grand_filler, self.env.num_envs,
                  stream)

    def choose(self, actions, model_of, reply_table, stream) -> None:
        _lib.call("ka_mate3_choose", self._records, self.root._records, self.cap, self.rows, self.third._records,
                  self.reply_cap, self.grand_terminated, self.grand_truncated, model_of, int(reply_table.shape[0]),
                  reply_table, self.root._child_err, self._grand_err, self.third._child_err, actions, self._counters,
                  self._counters.data_ptr() + 4 * self._nstats, self.env.num_envs, stream)

    def step(self, mask_bits, actions, model_of, table, reply_table, stream) -> None:
        """The root's three stages and the deeper ones behind them on the current stream (``stream``: its pointer), where
        ``MateSearch.step`` stands: ``actions`` (envs,) int64 is overwritten where a mate in one or in three replaces it.
        ``table`` the (K, 4) int32 controls table on the device, ``reply_table`` its ``mate3_reply_table``."""
        self.root.step(mask_bits, actions, model_of, table, stream)
        self.fork(mask_bits, actions, model_of, table, stream)
        self.step_grandchildren(stream)
        self.gate(model_of, stream)
        self.third.step(self.grand_mask_bits, self.grand_filler, self.grand_model_of, reply_table, stream)
        self.choose(actions, model_of, reply_table, stream)

    def read(self) -> Mate3Stats:
        """At a sync point: the counters since ``clear()`` (one small device -> host copy).  Raises on the error word."""
        self._counters_host.copy_(self._counters)
        c = self._counters_host.numpy()
        err = int(c[self._nstats])
        if err:
            which = [name for bit, name in ((ERR3_CHILD_STEP, "child"), (ERR3_GRAND_STEP, "grandchild"),
                                            (ERR3_THIRD_STEP, "third-ply")) if err & bit]
            raise RuntimeError(f"the mate search's {' and '.join(which)} step refused an action: a forked row does not "
                               "match the mask it was forked with")
        return Mate3Stats(*(int(v) for v in c[:self._nstats]))

    def records(self) -> torch.Tensor:
        """The per-env mate-in-three records of the last ``step`` (a copy on the device); ``root.records()`` are the
        mate-in-one records beside them, ``third.records()`` the third ply's, one per grandchild row."""
        return self._records.clone()


class MateStage(PlyStage):
    """The mate check as a loop builds it into its ply (``mate=``: a ``MateControls`` for every model, one per model, or a
    dict by model index), behind the lookahead or the search and before the insight: it overrides their choice, and the
    insight describes the move actually played.  The engine is a ``MateSearch`` whose child rows are sized by the largest
    ``max_checks`` given, or -- when a model's controls switch depth three on -- a ``Mate3Search`` (its ``root`` is that
    ``MateSearch``) with the grandchild and third-ply rows sized by the largest ``evasion_rows`` and ``reply_checks``; the
    stage then owns the third ply's ``reply_table`` too.  ``set_mate`` goes up to those sizes and switches depth three per
    model under the same capture.  ``RoundStats.mate`` carries the counters, ``RoundStats.mate3`` those of depth three."""

    name = "mate"
    _ABOVE, _ROWS = "the largest", "child, grandchild and third-ply rows"

    def __init__(self, table: np.ndarray, max_checks: int = 0, evasion_rows: int = 0, reply_checks: int = 0) -> None:
        deep = max_checks > 0 and evasion_rows > 0 and reply_checks > 0
        super().__init__(table, max_checks=int(max_checks), evasion_rows=int(evasion_rows) if deep else 0,
                         reply_checks=int(reply_checks) if deep else 0)
        self.reply_table: Optional[torch.Tensor] = None

    @classmethod
    def parse(cls, mate, num_models: int, collect: bool) -> Optional["MateStage"]:
        table, cap = arena_mate(mate, num_models, collect)
        return None if table is None else cls(table, cap, *arena_mate3(mate, num_models))

    @classmethod
    def _off(cls, num_models: int) -> "MateStage":
        return cls(mate_table(None, num_models))

    mate = property(lambda self: getattr(self.engine, "root", self.engine))             # the MateSearch, or None
    mate3 = property(lambda self: self.engine if self.sizes["evasion_rows"] else None)  # the Mate3Search, or None

    def _engine(self, env, group):
        cap, rows, reply = self.sizes.values()
        if rows:
            self.reply_table = torch.from_numpy(mate3_reply_table(self.host_table)).to(env.device)
            return Mate3Search(env, cap, rows, reply)
        return MateSearch(env, cap) if cap else None

    def _write(self, new: "MateStage") -> None:
        super()._write(new)
        if self.reply_table is not None:
            self.reply_table.copy_(torch.from_numpy(mate3_reply_table(new.host_table)))

    def _launch(self, logits, mask_bits, actions, model_of, seed, stream) -> None:
        tables = (self.table,) if self.reply_table is None else (self.table, self.reply_table)
        self.engine.step(mask_bits, actions, model_of, *tables, stream)

    def fresh(self) -> dict:
        return dict(mate=MateStats(), mate3=Mate3Stats()) if self.sizes["evasion_rows"] else dict(mate=MateStats())

    def _read(self) -> dict:
        return {field: getattr(self, field).read() for field in self.fresh()}

    def _record(self) -> dict:
        return {f"{field}_records": getattr(self, field).records().cpu() for field in self.fresh()}
