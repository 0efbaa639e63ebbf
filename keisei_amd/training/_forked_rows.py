"""What the searches of the device ply share on the Python side: the rows beneath an env (``ForkedRows``), the parser of a
per-model controls argument (``controls_rows``), the reader of a controls table (``table_of``), the field checks
(``check_int``, ``check_weight``), the check of the env and the group a search is built over (``check_search_env``) and the
shape in which a search is built into a ply (``PlyStage``).  ``Lookahead``, ``MateSearch`` and ``Mate3Search`` hold their
child and grandchild rows as ``ForkedRows``; ``TreeSearch`` and ``MctsSearch`` search in a ``NodePool``, a pool of slices
plus one scratch.  The device side of the same rows is csrc/ply_rows.h."""
from __future__ import annotations

import math
from typing import Callable, Dict, Mapping, Optional

import numpy as np
import torch

from keisei_amd import _lib
from keisei_amd.shogi_gym import ACTION_SPACE, MASK_WORDS

__all__ = ["ForkedRows", "NodePool", "PlyStage", "controls_rows", "table_of", "check_int", "check_weight",
           "check_search_env", "refuse_shared_place"]

ERR_VALUE, ERR_STEP = 1, 2                              # the error word of a node pool's advance


def check_int(name: str, v, lo: int, hi: int) -> int:
    """``v`` as an int when it is an integer in ``[lo, hi]`` and no bool; refused under ``name`` otherwise."""
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= v <= hi:
        raise ValueError(f"{name} must be an integer in [{lo}, {hi}], got {v!r}")
    return int(v)


def check_weight(name: str, w) -> float:
    """``w`` as a float when it is finite, >= 0 and fits a float32; refused under ``name`` otherwise."""
    if isinstance(w, bool) or not isinstance(w, (int, float)) or not math.isfinite(w) or w < 0:
        raise ValueError(f"{name} must be finite and >= 0, got {w!r}")
    if float(w) > 3.0e38:
        raise ValueError(f"{name} must fit a float32 (at most 3.0e38), got {w!r}")
    return float(w)


def check_search_env(env, group, what: str) -> None:
    """``what`` ("the lookahead", "the search", "the mate search") runs over a katago / spatial env with 128-byte state rows
    and, when it evaluates rows (``group`` not None), on a GPU group on the env's device."""
    if env._amode != 1 or env._omode != 1:
        raise ValueError(f"{what} covers the katago observation and the spatial action mode only")
    if group is not None:
        index = lambda d: torch.cuda.current_device() if d.index is None else d.index  # noqa: E731
        if getattr(group, "_tables", None) is None or group.device.type != "cuda" or index(group.device) != index(env.device):
            raise ValueError(f"{what} runs on a GPU group on the env's device ({env.device}); this group is on {group.device}")
    if env._state.shape[1] != 128:
        raise ValueError(f"{what} copies state rows of 128 bytes, the env's have {env._state.shape[1]}")


def controls_rows(controls, K, cls, what: str, by_index: bool = False) -> list:
    """K controls objects of class ``cls`` from ``controls``: None (K times ``cls.OFF``), one ``cls`` (every model), a
    sequence of exactly K or, with ``by_index``, a dict from model index to ``cls`` (a model not named is off).  ``what``
    names the argument in the errors ("lookahead", "search", "mate")."""
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or K < 1:
        raise ValueError(f"a {what} table needs at least one row, got K = {K!r}")
    K, name = int(K), cls.__name__
    if controls is None:
        return [cls.OFF] * K
    if isinstance(controls, cls):
        return [controls] * K
    if by_index and isinstance(controls, Mapping):
        extra = [k for k in controls if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= k < K]
        if extra:
            raise ValueError(f"{what} names model indices {extra} outside [0, {K})")
        rows = [controls.get(m, cls.OFF) for m in range(K)]
    elif isinstance(controls, (list, tuple)):
        rows = list(controls)
        if len(rows) != K:
            raise ValueError(f"expected {K} {name} (one per model), got {len(rows)}")
    else:
        forms = f"a {name}, a sequence of {K} or a dict by model index" if by_index else f"a {name} or a sequence of {K}"
        raise ValueError(f"{what} must be None, {forms}, got {type(controls).__name__}")
    for r in rows:
        if not isinstance(r, cls):
            raise ValueError(f"every entry must be a {name}, got {type(r).__name__}")
    return rows


def table_of(controls, K: Optional[int], make_table: Callable, what: str) -> np.ndarray:
    """The ``(K, 4)`` int32 table of ``controls``: a controls object or a sequence of them goes through ``make_table``
    (the module's ``*_table(controls, K)``; K None: the sequence's length, 1 for one object); an array or a tensor is a table
    as it lies in device memory and is taken as it is.  ``what`` names the table in the errors ("lookahead", "search")."""
    if isinstance(controls, torch.Tensor):
        controls = controls.detach().cpu().numpy()
    if isinstance(controls, np.ndarray):
        if controls.dtype != np.int32 or controls.ndim != 2 or controls.shape[1] != 4 or controls.shape[0] < 1:
            raise ValueError(f"a {what} table is a (K, 4) int32 array, got {controls.dtype} {controls.shape}")
        if K is not None and controls.shape[0] != K:
            raise ValueError(f"expected a table of {K} rows, got {controls.shape[0]}")
        return np.ascontiguousarray(controls)
    if K is None:
        K = len(controls) if isinstance(controls, (list, tuple)) else 1
    return make_table(controls, K)


def refuse_shared_place(**options) -> None:
    """The one rule between the searches: ``lookahead``, ``search`` and ``mcts`` stand in the same place in the ply (behind
    the sampler, before the mate check), and a ply plays the choice of one.  ``options``: what was given for each, in that
    order, None = not given; the later of two is refused."""
    given = [name for name, option in options.items() if option is not None]
    if len(given) > 1:
        raise ValueError(f"{given[-1]}= cannot be combined with {given[0]}=: the lookahead, the tree search and the "
                         "visit-count search stand in the same place in the ply, and a ply plays the choice of one")


class PlyStage:
    """One search as it is built into a ply: its ``name`` (the loop's keyword and the ``RoundStats`` field), its controls
    ``table`` on the device, its ``engine`` (None when every row of the table is off: the table exists, nothing is allocated
    and nothing is launched) and ``sizes``, what the engine's rows were sized by, by name.  A module's subclass says how the
    option is read (``parse``), how the engine is built (``_engine``) and launched (``_launch``), which ``RoundStats`` fields
    it fills (``fresh``, ``_read``) and what a recorded ply keeps of it (``_record``).  ``parse`` makes the stage on the
    host; ``DevicePly`` builds it on the device (``build``) and loops over its stages in ``reset()`` and ``move()``.  What a
    further search has to bring is such a subclass in its own module, its entry in ``MatchArena``'s stage list with a
    ``set_*`` one-liner, and its ``RoundStats`` field."""

    name = ""
    shares_place = False                                # it stands where the lookahead stands (``refuse_shared_place``)
    _ABOVE = "the {size}"                               # how ``rewrite`` names the built size it refuses to exceed
    _ROWS = "rows"                                      # ... and what was allocated by it

    def __init__(self, table: np.ndarray, **sizes: int) -> None:
        self.host_table, self.sizes = table, sizes
        self.table: Optional[torch.Tensor] = None
        self.engine = None

    @classmethod
    def parse(cls, option, num_models: int, collect: bool) -> Optional["PlyStage"]:
        """The stage of a loop's ``option`` on the host, through the module's ``arena_*`` reader; None for None."""
        raise NotImplementedError

    @classmethod
    def _off(cls, num_models: int) -> "PlyStage":
        raise NotImplementedError

    def build(self, env, group) -> None:
        """The table and, where a row is on, the engine, on the env's device; everything is allocated here, once."""
        self.table = torch.from_numpy(self.host_table).to(env.device)
        self.engine = self._engine(env, group)

    def rewriters(self) -> Dict[str, Callable]:
        """The loop's ``set_*`` options this stage answers, each with the method that takes ``(controls, num_models,
        collect)``."""
        return {self.name: self.rewrite}

    def rewrite(self, controls, num_models: int, collect: bool) -> None:
        """New controls from the next ply on; nothing is captured again.  None writes rows that are off.  Refused: what
        ``parse`` refuses (``collect=True``, a wrong row count) and a size above the one built, whose rows are allocated."""
        new = self.parse(controls, num_models, collect) or self._off(num_models)
        for size, built in self.sizes.items():
            if new.sizes[size] > built:
                raise ValueError(f"{self.name} {size} {new.sizes[size]} is above {self._ABOVE.format(size=size)} this arena "
                                 f"was built with ({built}): the {self._ROWS} are allocated once, by the largest {size} "
                                 "given to the constructor")
        with torch.cuda.device(self.table.device):
            self._write(new)

    def _write(self, new: "PlyStage") -> None:
        self.table.copy_(torch.from_numpy(new.host_table))

    def launch(self, logits, mask_bits, actions, model_of, seed: int, stream) -> None:
        """The stage's launches on the current stream (``stream``: its pointer), behind the sampler and before the env
        step: ``actions`` is overwritten for the envs the search decides.  ``seed``: the device pointer of the ply's seed."""
        if self.engine is not None:
            self._launch(logits, mask_bits, actions, model_of, seed, stream)

    def clear(self) -> None:
        if self.engine is not None:
            self.engine.clear()

    def fresh(self) -> dict:
        """The ``RoundStats`` fields the stage fills, as a round begins."""
        return {self.name: self.STATS()}

    def read(self) -> dict:
        """The same fields at a sync point, from the engine's counters; raises on its error word."""
        return self.fresh() if self.engine is None else self._read()

    def _read(self) -> dict:
        return {self.name: self.engine.read()}

    def record(self) -> dict:
        """What a recorded ply keeps of the stage's last launch (host copies)."""
        return {} if self.engine is None else self._record()


class NodePool:
    """The node pool of a device ``VecEnv`` that ``TreeSearch`` and ``MctsSearch`` search in, and the stages that move rows.
    Everything is allocated here, once: ``slices * envs * width`` node rows -- state, key and check history, both packed mask
    rows, action, model, policy logits, value logits and the step's scalars -- and one scratch of ``envs * width`` rows that
    every slice's step and forward write and nothing else reads: observations, terminal observations and the forward's
    activation maps.  Slice ``t`` of the pool is rows ``[t * envs * width, (t + 1) * envs * width)``; node ``(t, j)`` of env
    ``e`` is row ``(t * envs + e) * width + j``.  The trees, the principal variations and the counters (with the error
    word behind them, then ``extra_counters`` words of the subclass's) lie beside the pool; their sizes are the answers of the
    subclass's words query (``_WORDS``: 0 = words of a record, the lookahead's layout, 1 = of a tree, 2 = counters)."""

    _WORDS = ""                                             # the subclass's words query: ka_search_words, ka_mcts_words
    _WHAT, _SLICE = "the pool", "slice"                     # what a subclass calls itself and a slice in its errors

    def __init__(self, env, group, width: int, slices: int, extra_counters: int = 0) -> None:
        check_search_env(env, group, self._WHAT)
        q = lambda which: _lib.query(self._WORDS, which, width, slices)  # noqa: E731
        self.env, self.group, self.width, self.slices = env, group, width, slices
        self.words, self.tree_words, self._nstats = q(0), q(1), q(2)
        n, dev, hist = env.num_envs, env.device, env._keys.shape[1]
        self.M = M = n * width
        P = slices * M
        with torch.cuda.device(dev):
            z = lambda *shape, dtype: torch.zeros(*shape, dtype=dtype, device=dev)  # noqa: E731
            self.state = z(P, 128, dtype=torch.uint8)
            self.keys = z(P, hist, dtype=torch.int64)
            self.checks = z(P, hist, dtype=torch.uint8)
            self.bits_in = z(P, MASK_WORDS, dtype=torch.int32)         # the parents' masks: the step validates against them
            self.mask_bits = z(P, MASK_WORDS, dtype=torch.int32)
            self.actions = z(P, dtype=torch.int64)
            self.model_of = torch.full((P,), -1, dtype=torch.int32, device=dev)
            self.logits = z(P, 9, 9, ACTION_SPACE // 81, dtype=torch.float32)
            self.value_logits = z(P, 3, dtype=torch.float32)
            self.rewards = z(P, dtype=torch.float32)
            self.terminated = z(P, dtype=torch.bool)
            self.truncated = z(P, dtype=torch.bool)
            self.players = z(P, dtype=torch.uint8)
            self.reason = z(P, dtype=torch.uint8)
            self.captured = z(P, dtype=torch.uint8)
            self.ply = z(P, dtype=torch.int16)
            self.material = z(P, dtype=torch.int32)
            # the scratch of one slice, shared by all
            self.obs = z(M, env._C, 9, 9, dtype=torch.float32)
            self.terminal_obs = z(M, env._C, 9, 9, dtype=torch.float32)
            scratch = group._tables.workspace(M)
            self._ws = [dict(scratch, logits=self.logits[t * M:(t + 1) * M], value=self.value_logits[t * M:(t + 1) * M])
                        for t in range(slices)]
            self._env_stats = z(4, dtype=torch.int64)
            self._step_err = z(slices, 2, dtype=torch.int64)
            self._records = z(slices, n, self.words, dtype=torch.int32)
            self.parent_row = torch.full((n,), -1, dtype=torch.int32, device=dev)
            self.active = z(n, dtype=torch.int32)
            self._tree = z(n, self.tree_words, dtype=torch.int32)
            self._pv = torch.full((n, slices), -1, dtype=torch.int32, device=dev)
            self._counters = z(self._nstats + 1 + extra_counters, dtype=torch.int32)
            self._counters_host = torch.zeros(self._counters.shape, dtype=torch.int32).pin_memory()

    def clear(self) -> None:
        """Zero the counters, the error word and the refusal latches of every slice's step (a round's start)."""
        self._counters.zero_()
        self._step_err.zero_()

    def rows(self, t: int) -> slice:
        """The pool rows of slice ``t``."""
        if not 0 <= t < self.slices:
            raise ValueError(f"{self._SLICE} {t} lies outside [0, {self.slices})")
        return slice(t * self.M, (t + 1) * self.M)

    def node_row(self, e, node):
        """The pool row of local node ``node`` (``t * width + j``) of env ``e``."""
        return (node // self.width * self.env.num_envs + e) * self.width + node % self.width

    # ------------------------------------------------------------------ the stages that move rows
    def fork(self, logits, mask_bits, actions, model_of, table, stream) -> None:
        """Slice 0: the lookahead's fork of the envs."""
        env, s = self.env, self.rows(0)
        _lib.call("ka_lookahead_fork", logits, int(logits.dtype == torch.bfloat16), mask_bits, MASK_WORDS, actions, model_of,
                  int(table.shape[0]), table, env._state, env._keys, env._checks, env._max_ply, self.width, self._records[0],
                  self.state[s], self.keys[s], self.checks[s], self.bits_in[s], self.actions[s], self.model_of[s],
                  env.num_envs, ACTION_SPACE, stream)

    def expand(self, t: int, table, stream) -> None:
        """Slice ``t >= 1``, after ``advance(t - 1)``: the leaves named by ``parent_row`` / ``active`` fork into it."""
        env, s = self.env, self.rows(t)
        _lib.call("ka_search_expand", self.logits, 0, self.mask_bits, MASK_WORDS, self.model_of, int(table.shape[0]), table,
                  self.state, self.keys, self.checks, self.terminated, self.truncated, env._max_ply, self.width, t,
                  self.parent_row, self.active, self._records[t], self.state[s], self.keys[s], self.checks[s], self.bits_in[s],
                  self.actions[s], self.model_of[s], env.num_envs, ACTION_SPACE, stream)

    def step_nodes(self, t: int, stream) -> None:
        env, s = self.env, self.rows(t)
        _lib.call("ka_shogi_env_step", self.state[s], self.keys[s], self.checks[s], self.actions[s], self.M, env._max_ply,
                  env._omode, env._amode, None, self.bits_in[s], self._step_err[t], self.obs, None, self.mask_bits[s],
                  self.rewards[s], self.terminated[s], self.truncated[s], self.terminal_obs, self.players[s], self.captured[s],
                  self.reason[s], self.ply[s], self.material[s], self._env_stats, stream)

    def evaluate(self, t: int) -> None:
        self.group._tables.forward(self.obs, self.model_of[self.rows(t)], ws=self._ws[t])

    def step(self, logits, mask_bits, actions, model_of, table, stream) -> None:
        """Every stage on the current stream (``stream``: its pointer), after the sampler and before ``env.step``:
        ``actions`` (envs,) int64 is overwritten for the active envs.  Arguments as ``Lookahead.step``; ``table`` is the
        (K, 4) int32 table of the search on the device."""
        for t in range(self.slices):
            if t == 0:
                self.fork(logits, mask_bits, actions, model_of, table, stream)
            else:
                self.expand(t, table, stream)
            self.step_nodes(t, stream)
            self.evaluate(t)
            self.advance(t, actions, model_of, table, stream)

    def records(self, t=None) -> torch.Tensor:
        """The records of the last ``step`` (a copy on the device): (envs, 4 + 3 width) of slice ``t``, or all
        (slices, envs, 4 + 3 width)."""
        if t is None:
            return self._records.clone()
        self.rows(t)
        return self._records[t].clone()

    def principal_variations(self) -> torch.Tensor:
        """(envs, slices) int32: per env the chosen action and the line behind it, padded with -1."""
        return self._pv.clone()

    def _read_counters(self) -> np.ndarray:
        """At a sync point: the counters since ``clear()`` (one small device -> host copy).  Raises on the error word."""
        self._counters_host.copy_(self._counters)
        c = self._counters_host.numpy()
        err = int(c[self._nstats])
        if err & ERR_STEP:
            words = self._step_err.cpu()
            t = int(torch.nonzero(words.ne(0).any(1))[0]) if bool(words.ne(0).any()) else 0
            raise RuntimeError(f"{self._WHAT}'s step of {self._SLICE} {t} refused an action (word "
                               f"{int(words[t, 1]) or int(words[t, 0]):#x}): a forked row does not match the mask it was "
                               "forked with")
        if err & ERR_VALUE:
            raise RuntimeError(f"non-finite value logits in {self._WHAT} (a model has diverged)")
        return c


class ForkedRows:
    """``per_row`` rows beneath every row of ``parent`` (a device ``VecEnv`` or another ``ForkedRows``), allocated once: what
    ``ka_shogi_env_step`` reads and writes for them -- a state row, a key / check history row, the mask they are stepped
    against (``bits_in``), the action, and the step's outputs -- and, with a ``group``, a ``model_of`` column and a forward
    workspace.  A fork kernel fills ``state`` .. ``actions`` from ``parent_state`` .. ``parent_checks``; ``step`` steps them."""

    _NAMES = ("state", "keys", "checks", "bits_in", "actions", "obs", "mask_bits", "rewards", "terminated", "truncated",
              "players", "reason")

    def __init__(self, parent, per_row: int, group=None) -> None:
        above = isinstance(parent, ForkedRows)
        self.env = env = parent.env if above else parent
        self.parents = parent.M if above else env.num_envs
        self.parent_state, self.parent_keys, self.parent_checks = \
            (parent.state, parent.keys, parent.checks) if above else (env._state, env._keys, env._checks)
        self.M = M = self.parents * per_row
        dev, hist = env.device, env._keys.shape[1]
        with torch.cuda.device(dev):
            z = lambda *shape, dtype: torch.zeros(*shape, dtype=dtype, device=dev)  # noqa: E731
            self.state = z(M, 128, dtype=torch.uint8)
            self.keys = z(M, hist, dtype=torch.int64)
            self.checks = z(M, hist, dtype=torch.uint8)
            self.bits_in = z(M, MASK_WORDS, dtype=torch.int32)         # the parents' masks: the step validates against them
            self.actions = z(M, dtype=torch.int64)
            self.obs = z(M, env._C, 9, 9, dtype=torch.float32)
            self.mask_bits = z(M, MASK_WORDS, dtype=torch.int32)
            self.rewards = z(M, dtype=torch.float32)
            self.terminated = z(M, dtype=torch.bool)
            self.truncated = z(M, dtype=torch.bool)
            self.players = z(M, dtype=torch.uint8)
            self.reason = z(M, dtype=torch.uint8)
            self.terminal_obs = z(M, env._C, 9, 9, dtype=torch.float32)
            self.captured = z(M, dtype=torch.uint8)
            self.ply = z(M, dtype=torch.int16)
            self.material = z(M, dtype=torch.int32)
            self.env_stats = z(4, dtype=torch.int64)
            self.err = z(2, dtype=torch.int64)
            self.model_of = self.ws = None
            if group is not None:
                self.model_of = torch.full((M,), -1, dtype=torch.int32, device=dev)
                self.ws = group._tables.workspace(M)

    def step(self, stream) -> None:
        env = self.env
        _lib.call("ka_shogi_env_step", self.state, self.keys, self.checks, self.actions, self.M, env._max_ply, env._omode,
                  env._amode, None, self.bits_in, self.err, self.obs, None, self.mask_bits, self.rewards, self.terminated,
                  self.truncated, self.terminal_obs, self.players, self.captured, self.reason, self.ply, self.material,
                  self.env_stats, stream)

    def clear(self) -> None:
        """Zero the refusal latch of the step."""
        self.err.zero_()

    def alias(self, owner, prefix: str) -> None:
        """``owner.<prefix>_state`` .. ``owner.<prefix>_reason`` and ``owner._<prefix>_err``: the tensors under the names the
        searches have always shown them by; with a group also ``<prefix>_model_of``, ``_value_logits`` and ``_logits``."""
        for name in self._NAMES:
            setattr(owner, f"{prefix}_{name}", getattr(self, name))
        setattr(owner, f"_{prefix}_err", self.err)
        if self.ws is not None:
            setattr(owner, f"{prefix}_model_of", self.model_of)
            setattr(owner, f"{prefix}_value_logits", self.ws["value"])
            setattr(owner, f"{prefix}_logits", self.ws["logits"])
