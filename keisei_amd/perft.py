"""Perft of the device ``VecEnv``: fork every legal move of a frontier of positions, step the children with the env's own
step kernel, count (csrc/perft.hip; the reference's perft is shogi-core's, game.rs:1206-1222).

``VecEnv.perft`` / ``VecEnv.perft_divide`` are the public face; ``PerftWalk`` holds the rows and runs the walk.  The walk is
eager and host-driven, depth-first over chunks: level k holds at most ``rows`` complete env rows; ``ka_perft_plan`` takes as
many whole parents of level k as have room for their children in level k + 1, ``ka_perft_fork`` makes the children,
``ka_shogi_env_step`` (unchanged) steps exactly that many rows, ``ka_perft_tally`` counts them and their moves; the walk
descends, and afterwards moves the cursor of level k past the parents taken.  The host reads one 12-byte header per chunk.

Meaning: this is perft under the env's game rules -- a position in which the game has ended has no successors (the step
restarts such a row).  It equals the move-generation perft of the oracle's ``so_perft`` wherever no game in the tree ends
other than by checkmate; the "ended otherwise" column of ``by_depth`` says when that condition fails.
"""
from __future__ import annotations

import time
from dataclasses import dataclass
from typing import List, Tuple

import numpy as np
import torch

from . import _lib

__all__ = ["PerftResult", "PerftWalk", "perft_plan_host", "check_perft_args", "MAX_DEPTH", "MAX_MOVES", "MAX_ROWS", "COLUMNS"]

MAX_DEPTH = 8                      # ka_perft_words(4)
MAX_MOVES = 593                    # the most moves a legal shogi position has: ka_perft_words(2)
MAX_ROWS = 1 << 20                 # ka_perft_words(3)
COLUMNS = ("nodes", "mates", "ended_otherwise", "checks")      # by_depth[..., c]


@dataclass
class PerftResult:
    """``nodes`` (N,) uint64: the leaf count per env.  ``by_depth`` (N, depth, 4) uint64: per depth the nodes, the nodes
    whose game ended by checkmate, the ones it ended otherwise, and the nodes whose side to move is in check (the check byte
    of the row as the step left it: a row whose game ended holds the restarted game).  With ``bulk=True`` the last depth
    carries the nodes only.  ``chunks``: the number of fork launches."""
    nodes: np.ndarray
    by_depth: np.ndarray
    chunks: int


def perft_plan_host(moves, cursor: int, cap: int) -> Tuple[int, int, int, List[int]]:
    """``ka_perft_plan`` on the host: ``(taken, children, blocking, offsets)`` -- the longest run of whole parents from
    ``cursor`` whose moves sum to at most ``cap``, that sum, ``cursor + taken`` if the parent there has more than ``cap``
    moves by itself (else -1), and the first child row of each parent taken.  A negative count reads as 0."""
    n = len(moves)
    if not 0 <= cursor <= n:
        raise ValueError(f"cursor must lie in [0, {n}], got {cursor}")
    if not 1 <= cap <= MAX_ROWS:
        raise ValueError(f"cap must lie in [1, {MAX_ROWS}], got {cap}")
    taken, children, offsets = 0, 0, []
    for p in range(cursor, n):
        m = max(int(moves[p]), 0)
        if children + m > cap:
            break
        offsets.append(children)
        children += m
        taken += 1
    stop = cursor + taken
    return taken, children, (stop if stop < n and int(moves[stop]) > cap else -1), offsets


def check_perft_args(depth, rows) -> Tuple[int, int]:
    ok = lambda v: not isinstance(v, bool) and isinstance(v, (int, np.integer))  # noqa: E731
    if not ok(depth) or not 1 <= depth <= MAX_DEPTH:
        raise ValueError(f"depth must be an integer in [1, {MAX_DEPTH}], got {depth!r}")
    if not ok(rows) or not 1 <= rows <= MAX_ROWS:
        raise ValueError(f"rows must be an integer in [1, {MAX_ROWS}], got {rows!r}")
    return int(depth), int(rows)


class _Level:
    """The rows of one level that the next fork reads: state, history, the new mask, tag, moves and offset."""

    def __init__(self, n: int, hist: int, words: int, dev) -> None:
        z = lambda *shape, dtype: torch.zeros(*shape, dtype=dtype, device=dev)  # noqa: E731
        self.state = z(n, 128, dtype=torch.uint8)
        self.keys = z(n, hist, dtype=torch.int64)
        self.checks = z(n, hist, dtype=torch.uint8)
        self.mask = z(n, words, dtype=torch.int32)
        self.tag = z(n, dtype=torch.int32)
        self.moves = z(n, dtype=torch.int32)
        self.offset = z(n, dtype=torch.int32)


class PerftWalk:
    """The rows of a perft of ``depth`` levels of at most ``rows`` rows over a device ``VecEnv``, allocated here, once:
    per level what the next fork reads (``_Level``); the step's inputs and outputs nobody reads afterwards (the mask the
    children are stepped against, actions, observations, rewards and the rest) are one scratch of ``rows`` rows shared by all
    levels.  ``run`` walks the tree; ``last`` holds the launch counts and the seconds spent on header reads of the last run."""

    def __init__(self, env, depth: int, rows: int) -> None:
        from keisei_amd.training._forked_rows import check_search_env
        from keisei_amd.shogi_gym import ACTION_SPACE, MASK_WORDS
        check_search_env(env, None, "perft")
        depth, rows = check_perft_args(depth, rows)
        assert _lib.query("ka_perft_words", 0) == len(COLUMNS) and _lib.query("ka_perft_words", 1) == 3
        assert _lib.query("ka_perft_words", 2) == MAX_MOVES and _lib.query("ka_perft_words", 3) == MAX_ROWS
        assert _lib.query("ka_perft_words", 4) == MAX_DEPTH
        self.env, self.depth, self.rows = env, depth, rows
        self._A, self._words = ACTION_SPACE, MASK_WORDS
        n, dev, hist = env.num_envs, env.device, env._keys.shape[1]
        with torch.cuda.device(dev):
            z = lambda *shape, dtype: torch.zeros(*shape, dtype=dtype, device=dev)  # noqa: E731
            self.levels = [_Level(rows, hist, MASK_WORDS, dev) for _ in range(depth)]      # levels 1 .. depth
            self.tag0, self.moves0, self.offset0 = (z(n, dtype=torch.int32) for _ in range(3))
            self.tag0.copy_(torch.arange(n, dtype=torch.int32))
            self.bits_in = z(rows, MASK_WORDS, dtype=torch.int32)
            self.actions = z(rows, dtype=torch.int64)
            self.obs = z(rows, env._C, 9, 9, dtype=torch.float32)
            self.terminal_obs = z(rows, env._C, 9, 9, dtype=torch.float32)
            self.rewards = z(rows, dtype=torch.float32)
            self.terminated = z(rows, dtype=torch.bool)
            self.truncated = z(rows, dtype=torch.bool)
            self.players = z(rows, dtype=torch.uint8)
            self.captured = z(rows, dtype=torch.uint8)
            self.reason = z(rows, dtype=torch.uint8)
            self.ply = z(rows, dtype=torch.int16)
            self.material = z(rows, dtype=torch.int32)
            self.env_stats = z(4, dtype=torch.int64)
            self.step_err = z(2, dtype=torch.int64)
            self.fork_err = z(1, dtype=torch.int32)
            self.header = z(3, dtype=torch.int32)
            self._header_host = torch.zeros(3, dtype=torch.int32).pin_memory()
        self.last: dict = {}

    # ------------------------------------------------------------------ stages
    def _plan(self, moves, cursor: int, n: int, offset) -> Tuple[int, int, int]:
        _lib.call("ka_perft_plan", moves, cursor, n, self.rows, offset, self.header, self._stream)
        t0 = time.perf_counter()
        self._header_host.copy_(self.header)                  # (a blocking copy: everything queued so far has run)
        self.last["header_seconds"] += time.perf_counter() - t0
        self.last["plans"] += 1
        h = self._header_host.numpy()
        return int(h[0]), int(h[1]), int(h[2])

    def _tally(self, state, mask, ended, tag, n: int, level: int, leaf: bool, moves) -> None:
        term, trunc, reason = ended
        _lib.call("ka_perft_tally", state, mask, self._words, term, trunc, reason, tag, n, level, self.depth, int(leaf),
                  self._tags, moves, self._tally_table, self._leaves, self._stream)
        self.last["tallies"] += 1

    def _walk(self, k: int, n: int, parent) -> None:
        """Fork the n rows of level k (``parent``: state, keys, checks, mask, tag, moves, offset) into level k + 1, chunk by
        chunk, and descend."""
        env, child = self.env, self.levels[k]
        p_state, p_keys, p_checks, p_mask, p_tag, p_moves, p_offset = parent
        cursor = 0
        while cursor < n:
            taken, children, blocking = self._plan(p_moves, cursor, n, p_offset)
            if blocking >= 0:
                m = int(p_moves[blocking].item())
                raise ValueError(f"row {blocking} of level {k} has {m} legal moves and rows={self.rows} has no room for them: "
                                 f"give perft at least rows={MAX_MOVES}, the most moves a legal shogi position has")
            if taken <= 0:
                raise RuntimeError(f"perft: the plan of level {k} took no parent at cursor {cursor} of {n}")
            if children > 0:
                base = -1
                if self._divide and k == 0:
                    base, self._ordinal = self._ordinal, self._ordinal + children
                _lib.call("ka_perft_fork", p_state, p_mask, self._words, p_keys, p_checks, p_moves, p_offset, p_tag, cursor,
                          taken, n, env._max_ply, self.rows, base, child.state, child.keys, child.checks, self.bits_in,
                          self.actions, child.tag, self.fork_err, self._A, self._stream)
                _lib.call("ka_shogi_env_step", child.state, child.keys, child.checks, self.actions, children, env._max_ply,
                          env._omode, env._amode, None, self.bits_in, self.step_err, self.obs, None, child.mask, self.rewards,
                          self.terminated, self.truncated, self.terminal_obs, self.players, self.captured, self.reason,
                          self.ply, self.material, self.env_stats, self._stream)
                self.last["forks"] += 1
                self.last["steps"] += 1
                last = k + 1 == self._forked
                self._tally(child.state, child.mask, (self.terminated, self.truncated, self.reason), child.tag, children, k,
                            last and self._bulk, child.moves)
                if not last:
                    self._walk(k + 1, children,
                               (child.state, child.keys, child.checks, child.mask, child.tag, child.moves, child.offset))
            cursor += taken

    # ------------------------------------------------------------------ the walk
    def run(self, depth: int, bulk: bool = True, divide: bool = False):
        """Perft to ``depth`` (at most the depth the rows were made for) of the env's positions to move.  Returns
        ``(tally, leaves)`` as host uint64 arrays of shapes (T, self.depth, 4) and (T,), where a tag is an env (T = N) or,
        with ``divide``, a child of the first level in (env, ascending action) order.  The env is only read."""
        if not 1 <= depth <= self.depth:
            raise ValueError(f"these rows serve depths 1..{self.depth}, got {depth}")
        env = self.env
        n = env.num_envs
        with torch.cuda.device(env.device):
            self._stream = _lib.stream_ptr()
            self._bulk, self._divide, self._ordinal = bool(bulk), bool(divide), 0
            self._forked = depth - 1 if bulk else depth           # the levels that are forked and stepped
            self.last = {"plans": 0, "forks": 0, "steps": 0, "tallies": 0, "header_seconds": 0.0, "seconds": 0.0}
            t0 = time.perf_counter()
            self.fork_err.zero_()
            self.step_err.zero_()
            bits = env._bits[env._cur]
            # level 0: the env's own rows; their moves, and with nothing to fork their moves are the leaves
            self._tags = n
            self._tally_table = torch.zeros(n, self.depth, len(COLUMNS), dtype=torch.int64, device=env.device)
            self._leaves = torch.zeros(n, dtype=torch.int64, device=env.device)
            self._tally(env._state, bits, (None, None, None), self.tag0, n, -1, self._forked == 0 and bulk, self.moves0)
            if divide:                                            # a tag per child of the first level
                self._tags = max(int(self.moves0.sum().item()), 1)
                self._tally_table = torch.zeros(self._tags, self.depth, len(COLUMNS), dtype=torch.int64, device=env.device)
                self._leaves = torch.zeros(self._tags, dtype=torch.int64, device=env.device)
            if self._forked > 0:
                self._walk(0, n, (env._state, env._keys, env._checks, bits, self.tag0, self.moves0, self.offset0))
            tally = self._tally_table.cpu().numpy().view(np.uint64)
            leaves = self._leaves.cpu().numpy().view(np.uint64)
            err, step_err = int(self.fork_err.item()), int(self.step_err[1].item())
            self.last["seconds"] = time.perf_counter() - t0
            self._tally_table = self._leaves = None
        if step_err:
            raise RuntimeError(f"perft's child step refused an action (word {step_err:#x}): a forked row does not match the "
                               "mask it was forked with")
        if err:
            raise RuntimeError(f"perft's fork reported error {err:#x} (1: children outside their level's rows, 2: a mask that "
                               "does not match the moves counted from it)")
        return tally, leaves

    def perft(self, depth: int, bulk: bool = True) -> PerftResult:
        tally, leaves = self.run(depth, bulk, False)
        by_depth = np.ascontiguousarray(tally[:, :depth])
        if bulk:
            by_depth[:, depth - 1, 0] = leaves
        return PerftResult(by_depth[:, depth - 1, 0].copy(), by_depth, self.last["forks"])

    def divide(self, depth: int) -> List[dict]:
        env = self.env
        bits = env._bits[env._cur].cpu().numpy().view(np.uint8)
        legal = np.unpackbits(bits, axis=1, bitorder="little")[:, :self._A]
        actions = [np.flatnonzero(row) for row in legal]
        if depth == 1:
            return [{int(a): 1 for a in acts} for acts in actions]
        _, leaves = self.run(depth, True, True)
        out, o = [], 0
        for acts in actions:
            out.append({int(a): int(leaves[o + j]) for j, a in enumerate(acts)})
            o += len(acts)
        return out
