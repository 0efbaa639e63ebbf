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
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import ClassVar, Mapping, Optional, Tuple

import numpy as np
import torch

from keisei_amd import _lib
from keisei_amd.shogi_gym import ACTION_SPACE, MASK_WORDS

__all__ = ["MateControls", "MateStats", "MateSearch", "mate_table", "mate_words", "arena_mate", "MAX_CHECKS",
           "MAX_SKIP_PLIES"]

MAX_CHECKS = 64
MAX_SKIP_PLIES = 65535
# record words (csrc/mate.hip; ka_mate_words reports the sizes)
REC_FLAGS, REC_NCHECKS, REC_SLOT, REC_ACTION, REC_LIST = 0, 1, 2, 3, 4
FLAG_ACTIVE, FLAG_MATE, FLAG_CHANGED, FLAG_TRUNCATED = 1, 2, 4, 8
ERR_CHILD_STEP = 2


def mate_words(cap: int) -> int:
    """32-bit words of one record."""
    return REC_LIST + int(cap)


@dataclass(frozen=True)
class MateControls:
    """One model's mate-in-one controls.  ``max_checks`` 0 is off."""
    max_checks: int = 16
    skip_plies: int = 0

    OFF: ClassVar["MateControls"]

    def __post_init__(self) -> None:
        for name, hi in (("max_checks", MAX_CHECKS), ("skip_plies", MAX_SKIP_PLIES)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= hi:
                raise ValueError(f"{name} must be an integer in [0, {hi}], got {v!r}")
            object.__setattr__(self, name, int(v))

    def row(self) -> np.ndarray:
        """The table row: int32 max_checks, int32 skip_plies, two reserved zero words."""
        return np.array([self.max_checks, self.skip_plies, 0, 0], dtype=np.int32)


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
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or K < 1:
        raise ValueError(f"a mate table needs at least one row, got K = {K!r}")
    K = int(K)
    if controls is None:
        return [MateControls.OFF] * K
    if isinstance(controls, MateControls):
        return [controls] * K
    if isinstance(controls, Mapping):                  # model index -> controls; a model not named is off
        extra = [k for k in controls if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= k < K]
        if extra:
            raise ValueError(f"mate names model indices {extra} outside [0, {K})")
        rows = [controls.get(m, MateControls.OFF) for m in range(K)]
    elif isinstance(controls, (list, tuple)):
        rows = list(controls)
        if len(rows) != K:
            raise ValueError(f"expected {K} MateControls (one per model), got {len(rows)}")
    else:
        raise ValueError(f"mate must be None, a MateControls, a sequence of {K} or a dict by model index, "
                         f"got {type(controls).__name__}")
    for r in rows:
        if not isinstance(r, MateControls):
            raise ValueError(f"every entry must be a MateControls, got {type(r).__name__}")
    return rows


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


def _check_cap(cap) -> int:
    if isinstance(cap, bool) or not isinstance(cap, (int, np.integer)) or not 1 <= cap <= MAX_CHECKS:
        raise ValueError(f"cap must be an integer in [1, {MAX_CHECKS}], got {cap!r}")
    return int(cap)


class MateSearch:
    """The child rows of a device ``VecEnv`` and the three stages of the mate check.  Everything is allocated here, once:
    ``cap`` child rows per env, each a state row, a key / check history row, two packed mask rows and the step's outputs
    (the rows the lookahead holds per child, minus the forward workspace: no forward runs here).  ``records()``
    (envs, 4 + cap) int32 are the envs' records of the last ``step``."""

    def __init__(self, env, cap: int) -> None:
        cap = _check_cap(cap)
        if env._amode != 1 or env._omode != 1:
            raise ValueError("the mate search covers the katago observation and the spatial action mode only")
        if env._state.shape[1] != 128:
            raise ValueError(f"the mate search copies state rows of 128 bytes, the env's have {env._state.shape[1]}")
        self.env, self.cap = env, cap
        n, dev, hist = env.num_envs, env.device, env._keys.shape[1]
        self.words = _lib.query("ka_mate_words", 0, cap)
        assert self.words == mate_words(cap) and cap <= _lib.query("ka_mate_words", 3, 0) == MAX_CHECKS
        self.M = M = n * cap
        with torch.cuda.device(dev):
            z = lambda *shape, dtype: torch.zeros(*shape, dtype=dtype, device=dev)  # noqa: E731
            self._records = z(n, self.words, dtype=torch.int32)
            self.child_state = z(M, 128, dtype=torch.uint8)
            self.child_keys = z(M, hist, dtype=torch.int64)
            self.child_checks = z(M, hist, dtype=torch.uint8)
            self.child_bits_in = z(M, MASK_WORDS, dtype=torch.int32)       # the parents' masks: the step validates against them
            self.child_actions = z(M, dtype=torch.int64)
            self.child_obs = z(M, env._C, 9, 9, dtype=torch.float32)
            self.child_mask_bits = z(M, MASK_WORDS, dtype=torch.int32)
            self.child_rewards = z(M, dtype=torch.float32)
            self.child_terminated = z(M, dtype=torch.bool)
            self.child_truncated = z(M, dtype=torch.bool)
            self.child_players = z(M, dtype=torch.uint8)
            self.child_reason = z(M, dtype=torch.uint8)
            self._terminal_obs = z(M, env._C, 9, 9, dtype=torch.float32)
            self._captured = z(M, dtype=torch.uint8)
            self._ply = z(M, dtype=torch.int16)
            self._material = z(M, dtype=torch.int32)
            self._env_stats = z(4, dtype=torch.int64)
            self._child_err = z(2, dtype=torch.int64)
            self._counters = z(_lib.query("ka_mate_words", 2, cap), dtype=torch.int32)       # stats, then the error word
            self._counters_host = torch.zeros(self._counters.shape, dtype=torch.int32).pin_memory()
        self._nstats = self._counters.shape[0] - 1

    def clear(self) -> None:
        """Zero the counters, the error word and the refusal latch of the child step (a round's start)."""
        self._counters.zero_()
        self._child_err.zero_()

    def fork(self, mask_bits, actions, model_of, table, stream) -> None:
        env = self.env
        _lib.call("ka_mate_fork", mask_bits, MASK_WORDS, actions, model_of, int(table.shape[0]), table, env._state, env._keys,
                  env._checks, env._max_ply, self.cap, self._records, self.child_state, self.child_keys, self.child_checks,
                  self.child_bits_in, self.child_actions, env.num_envs, ACTION_SPACE, stream)

    def step_children(self, stream) -> None:
        env = self.env
        _lib.call("ka_shogi_env_step", self.child_state, self.child_keys, self.child_checks, self.child_actions, self.M,
                  env._max_ply, env._omode, env._amode, None, self.child_bits_in, self._child_err, self.child_obs, None,
                  self.child_mask_bits, self.child_rewards, self.child_terminated, self.child_truncated, self._terminal_obs,
                  self.child_players, self._captured, self.child_reason, self._ply, self._material, self._env_stats, stream)

    def choose(self, actions, stream) -> None:
        _lib.call("ka_mate_choose", self._records, self.cap, self.child_rewards, self.child_terminated, self.child_reason,
                  self._child_err, actions, self._counters, self._counters.data_ptr() + 4 * self._nstats, self.env.num_envs,
                  stream)

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
