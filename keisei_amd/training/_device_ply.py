"""The device-resident ply that ``MatchArena``, ``LeagueRollout`` and ``SelfPlayRollout`` share, and the skeleton of the
two loops that write a rollout buffer.

``DevicePly`` is what one ply of any of the three does before its own bookkeeping launch: the grouped forward, the
sampler, the optional searches (a list of ``PlyStage``) and insight, the env step and the optional game-log launch.  A loop holds one by
composition and adds its state array, its ``model_of`` and its bookkeeping kernel (``ka_arena_referee``,
``ka_league_step``, ``ka_selfplay_step``).  ``DeviceRollout`` is the part of ``LeagueRollout`` and ``SelfPlayRollout``
around the ply: graph capture per buffer parity, the column descriptor, the guard decoding of a sync point, the learner's
value forward, the buffer checks of ``collect()``.  The arena keeps its own capture (one reset per round, so one parity)
and its own state layout.
"""
from __future__ import annotations

import gc
import math
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from keisei_amd import _lib
from keisei_amd.shogi_gym import ACTION_SPACE, MASK_WORDS, OBS_CHANNELS, VecEnv

from ._forked_rows import PlyStage, refuse_shared_place
from .game_log import GameLog, RecordedGame
from .katago_ppo import KataGoRolloutBuffer, _check_step_inputs
from .policy_insight import InsightRecorder
from .sampling import GAME_PLY_BYTE
from .search_samples import SearchSamples
from .value_adapter import MultiHeadValueAdapter

_OBS_SHAPE = (OBS_CHANNELS, 9, 9)
_OBS_ELEMS = OBS_CHANNELS * 81          # one observation row as the env hands it over (fp32)
# the words of the state array that csrc/league.hip and csrc/selfplay.hip lay out alike (the arena's differ)
_SEED, _PLY, _ROWS, _DROPPED, _SAMP, _REFUSAL, _TRUNC, _TRUNC_DROPPED = 0, 2, 3, 5, 6, 8, 12, 13
_WINS, _LOSSES, _DRAWS, _BLACK, _WHITE, _TERMINATED, _TRUNCATED, _GUARDS = 14, 15, 16, 17, 18, 19, 20, 21
# the column pointers of the rollout store in the order of the kernels' descriptor; words 12, 13: base row, reserved rows
_DESC_KEYS = ("observations", "legal_masks", "actions", "log_probs", "values", "rewards", "dones", "terminated",
              "value_categories", "score_targets", "env_ids", "next_value_override")


def check_loop_args(max_ply: int, sync_every: int, graph: bool, record: bool, start_pool_capacity: int = 0,
                    game_log: int = 0, *, one_truncation_slot: bool = False) -> None:
    """The geometry every loop checks.  ``one_truncation_slot``: the rollouts park one truncated game per env and sync
    point, so their ``sync_every`` must not exceed ``max_ply``."""
    if not 1 <= max_ply <= 65535:
        raise ValueError(f"max_ply must lie in [1, 65535], got {max_ply}")
    if sync_every < 1:
        raise ValueError(f"sync_every must be at least 1, got {sync_every}")
    if one_truncation_slot and sync_every > max_ply:
        raise ValueError(f"sync_every ({sync_every}) must not exceed max_ply ({max_ply}): an env may truncate only once "
                         "between two sync points (one truncation slot per env)")
    if graph and record:
        raise ValueError("record=True runs without a graph (graph=False)")
    if graph and sync_every % 2:
        raise ValueError(f"graph=True needs an even sync_every (VecEnv alternates two result buffers), got {sync_every}")
    if start_pool_capacity < 0:
        raise ValueError(f"start_pool_capacity must not be negative, got {start_pool_capacity}")
    if game_log < 0:
        raise ValueError(f"game_log must not be negative, got {game_log}")


def check_value_args(score_norm: float, value_adapter) -> None:
    if not math.isfinite(score_norm) or score_norm == 0:
        raise ValueError(f"score_norm must be finite and non-zero, got {score_norm}")
    if value_adapter is not None and type(value_adapter) is not MultiHeadValueAdapter:
        raise ValueError(f"value_adapter must be None or a MultiHeadValueAdapter (the kernel blends by its "
                         f"score_blend_alpha), got {type(value_adapter).__name__}")


class DevicePly:
    """One device ``VecEnv``, the rows a ply writes (``actions``, ``log_probs``, ``n_legal``), the forward workspace and
    the optional parts of a ply.  The options, as every loop's constructor takes them:

    ``start_pool_capacity > 0`` gives the env a pool of start positions of that size: ``loop.env.set_start_positions(...)``
    / ``set_start_sfens(...)`` between two collections make later games start from them (no re-capture; see ``VecEnv``).
    ``game_log=K > 0`` adds a device-resident ``GameLog`` of K records to the ply (one launch, ``ka_gamelog_step`` or
    ``ka_gamelog_step_env``, between the env step and the loop's bookkeeping launch); the loop drains it at every sync
    point, and ``live_games()`` between two collections gives the games still in progress.  ``move_history=True`` has the
    env keep the move notes of the games in progress (two more launches inside ``env.step``, see ``VecEnv``);
    ``spectator_data()`` between two collections is the dashboard feed either way.  ``insight=top_k > 0`` adds the policy
    insight to the ply (one launch, ``ka_policy_insight``, between the sampler and the env step; ``policy_insight.py``):
    every ``spectator_data()`` dict gains ``insight``, the figures of the env's last move at ``insight_temperature``, and
    with ``move_history=True`` every history entry gains its move's probability, rank, entropy, win probability and top
    candidates.  ``controls`` (a table of ``sampling.py``) puts ``ka_policy_sample_ctl`` in the place of
    ``ka_policy_sample_play``.  ``stages`` are the searches of the ply, in launch order: ``PlyStage`` objects as their
    modules parse a loop's options (``lookahead.py``, ``tree_search.py``, ``mcts_search.py``, ``mate_search.py``; a None
    among them is an option not given).  They are built here, launched between the sampler and the insight, cleared by
    ``reset()`` and kept by name in ``self.stages``; at most one of them may stand in the lookahead's place.
    ``search_samples=rows_per_env > 0`` (only with the visit-count search; ``search_samples.py``) keeps the searched
    positions with their visit counts and, once the game has ended, its result as training rows on the device: one launch,
    ``ka_search_sample_step``, that the loop enqueues through ``sample(...)`` between the env step and its bookkeeping launch.
    An option left at 0 / None adds no launch and allocates nothing."""

    def __init__(self, group, num_envs: int, max_ply: int, *, start_pool_capacity: int = 0, game_log: int = 0,
                 envs_per_slot: Optional[int] = None, move_history: bool = False, insight: int = 0,
                 insight_temperature: float = 1.0, controls: Optional[np.ndarray] = None,
                 stages: Sequence[Optional[PlyStage]] = (), search_samples: int = 0) -> None:
        self.stages: Dict[str, PlyStage] = {s.name: s for s in stages if s is not None}
        refuse_shared_place(**{name: s for name, s in self.stages.items() if s.shares_place})
        N, dev = int(num_envs), group.device
        self.device, self.num_envs = dev, N
        with torch.cuda.device(dev):
            self.env = VecEnv(N, int(max_ply), "katago", "spatial", device=dev, output="torch", check_actions=False,
                              start_pool_capacity=int(start_pool_capacity), move_history=bool(move_history))
            self.actions = torch.zeros(N, dtype=torch.int64, device=dev)
            self.log_probs = torch.zeros(N, dtype=torch.float32, device=dev)
            self.n_legal = torch.zeros(N, dtype=torch.int32, device=dev)
            self.game_log: Optional[GameLog] = None
            if game_log:
                self.game_log = GameLog(self.env, capacity=int(game_log), envs_per_slot=envs_per_slot)
            self.insight: Optional[InsightRecorder] = InsightRecorder(self.env, insight, insight_temperature) if insight else None
            # every stage's table (read by every launch) and its rows, allocated once
            for stage in self.stages.values():
                stage.build(self.env, group)
            self.mcts = getattr(self.stages.get("mcts"), "engine", None)      # the visit-count search: its visits are read
            # the samples of the visit-count search: a region of rows per env, allocated once
            self.search_samples: Optional[SearchSamples] = None
            if search_samples:
                if self.mcts is None:
                    raise ValueError("search_samples needs the visit-count search (an mcts stage with a width above 0): a "
                                     "sample is a searched position with its visit counts")
                self.search_samples = SearchSamples(self.env, self.mcts, search_samples)
            self.seat(group, controls)

    def seat(self, group, controls: Optional[np.ndarray]) -> None:
        """The group the forward runs (a new workspace) and the controls table of ``ka_policy_sample_ctl`` (None: the play
        sampler).  A loop that calls this again drops its captured graphs."""
        self.group = group
        with torch.cuda.device(self.device):
            self.ws = group._tables.workspace(self.num_envs)
            self.ctl: Optional[torch.Tensor] = None if controls is None else torch.from_numpy(controls).to(self.device)

    def reset(self) -> None:
        """Every env back to the start position; the log, the insight and the stages' counters begin anew."""
        self.env.reset()
        if self.game_log is not None:
            self.game_log.begin()
        if self.insight is not None:
            self.insight.clear()
        for stage in self.stages.values():
            stage.clear()
        if self.search_samples is not None:
            self.search_samples.begin()

    def move(self, model_of: torch.Tensor, num_models: int, state: int, flags: int):
        """forward -> sampler -> the stages, in their order -> insight on the current stream.  ``state``: the device pointer of the loop's
        state array (the sampler reads the seed at its head), ``flags``: of the two sampler-flag words in it.  Returns
        ``(cur, pre, value, score, stream)``: the env's current buffers, the players to move, the value logits and the
        score lead of the forward, and the stream's pointer for the launches that follow."""
        env, N = self.env, self.num_envs
        st = _lib.stream_ptr(self.device)
        cur, pre = env.current(), env._players[env._cur]
        logits, value, score = self.group._tables.forward(cur.observations, model_of, ws=self.ws)
        if self.ctl is None:
            _lib.call("ka_policy_sample_play", logits, 0, cur.legal_mask_bits, MASK_WORDS, state, model_of, num_models,
                      self.actions, self.log_probs, self.n_legal, flags, N, ACTION_SPACE, st)
        else:                                             # the game ply of the position to move in: byte 100 of the state row
            _lib.call("ka_policy_sample_ctl", logits, 0, cur.legal_mask_bits, MASK_WORDS, state, model_of, num_models,
                      self.ctl, env._state.data_ptr() + GAME_PLY_BYTE, env._state.shape[1], self.actions, self.log_probs,
                      self.n_legal, flags, N, ACTION_SPACE, st)
        for stage in self.stages.values():                # the active envs' actions become the search's choices; a later
            stage.launch(logits, cur.legal_mask_bits, self.actions, model_of, state, st)      # stage overrides an earlier one
        if self.insight is not None:                      # while the logits exist, before the step moves the history count
            self.insight.step(logits, cur.legal_mask_bits, self.actions, value, pre, model_of, num_models, flags, st)
        return cur, pre, value, score, st

    def step(self):
        """``env.step`` on the chosen actions."""
        return self.env.step(self.actions)

    def log(self, r, pre: torch.Tensor, **kw) -> None:
        """The game-log launch behind the env step ``r``, before the loop's bookkeeping launch rewrites what the log reads.
        ``kw``: how the loop names the players (the arena's ``pairs=`` / ``live=``, the league's ``side=`` / ``opp=`` /
        ``ids=``, which takes the per-env form of the launch) and its ``ply_counter=``."""
        if self.game_log is not None:
            fn = self.game_log.step_env if "ids" in kw else self.game_log.step
            fn(self.actions, r.rewards, r.terminated, r.truncated, pre, r.step_metadata.termination_reason,
               nlegal=self.n_legal, **kw)

    def sample(self, r, pre: torch.Tensor, model_of: torch.Tensor, stream) -> None:
        """The search-sample launch behind the env step ``r``, before the loop's bookkeeping launch rewrites ``model_of``:
        the position before the move lies in the env's previous buffers, ``pre`` are its players to move."""
        if self.search_samples is not None:
            env = self.env
            self.search_samples.step(env._obs[env._cur ^ 1], pre, model_of, self.actions, r.step_metadata.material_balance,
                                     r.rewards, r.terminated, r.truncated, stream)

    def live_games(self, owner: str, envs: Optional[Sequence[int]], **kw) -> List[RecordedGame]:
        if self.game_log is None:
            raise ValueError(f"live_games() needs {owner} built with game_log > 0")
        with torch.cuda.device(self.device):
            return self.game_log.live(envs, **kw)

    def spectator_data(self, envs: Optional[Sequence[int]] = None, values: Optional[torch.Tensor] = None) -> List[dict]:
        """``VecEnv.get_spectator_data`` of every env (or ``envs``); ``move_history`` is [] unless built with
        ``move_history=True``; ``insight`` (built with ``insight > 0``) is the ``insight_dict`` of the env's last move, None
        before its first move after a reset.  ``values`` (envs,): every dict gains its env's as ``value_estimate``."""
        with torch.cuda.device(self.device):
            data = self.env.get_spectator_data(envs)
            if values is not None:
                host = values.cpu().numpy()
                for d, e in zip(data, range(self.num_envs) if envs is None else [int(e) for e in envs]):
                    d["value_estimate"] = float(host[e])
            return data if self.insight is None else self.insight.annotate(data, envs)


class DeviceRollout:
    """What ``LeagueRollout`` and ``SelfPlayRollout`` share around their ply.  A subclass sets ``_LAYOUT`` (its kernel's
    layout query: 0 = plan words, 1 = descriptor words) and ``_ENV_IDS`` (the buffer layout it reserves), builds
    ``self.ply`` through ``_build`` and provides ``_ply``, ``_ply_recorded``, ``_zero_legal``, ``_overrides`` and ``_collect``."""

    _LAYOUT = ""
    _ENV_IDS = True
    _DIVERGED = "a model"                               # who the NaN-logits message blames
    _SAMP, _REFUSAL = _SAMP, _REFUSAL                   # state words: the sampler's two flags, the env's refusal latch

    def _build(self, group, *, num_envs, max_ply, sync_every, graph, seed, record, value_adapter, score_norm,
               trunc_words: int, **ply_options) -> None:
        """The fields and buffers both loops hold; the state array is the subclass's (its size may follow a cohort)."""
        self.group, self.device = group, group.device
        self.num_envs, self.max_ply, self.sync_every = int(num_envs), int(max_ply), int(sync_every)
        self.graph, self.seed, self.record_enabled = bool(graph), seed, bool(record)
        self.value_adapter, self.score_norm = value_adapter, float(score_norm)
        self.alpha = 0.0 if value_adapter is None else float(value_adapter.score_blend_alpha)
        self.record: List[dict] = []
        N, dev = self.num_envs, self.device
        self.ply = DevicePly(group, N, self.max_ply, **ply_options)
        self.env, self.game_log, self.insight = self.ply.env, self.ply.game_log, self.ply.insight
        self._actions, self._logp, self._nlegal = self.ply.actions, self.ply.log_probs, self.ply.n_legal
        q = lambda which: _lib.query(self._LAYOUT, which)  # noqa: E731
        with torch.cuda.device(dev):
            z = lambda *s, dtype=torch.int32: torch.zeros(*s, dtype=dtype, device=dev)  # noqa: E731
            self._values = z(N, dtype=torch.float32)
            self._model_of, self._learner_of = z(N), z(N)        # the rows of the ply to come; every row on model 0
            self._stall = z(N, dtype=torch.uint8)
            self._t_obs, self._t_list = z(N, *_OBS_SHAPE, dtype=torch.float32), z(N, trunc_words)
            self._plan = z(N, q(0))
            self._desc = z(q(1), dtype=torch.int64)
            self._desc_host = torch.zeros(q(1), dtype=torch.int64).pin_memory()
        self._graphs: Dict[int, torch.cuda.CUDAGraph] = {}

    def _new_state(self, words: int) -> None:
        with torch.cuda.device(self.device):
            self._state = torch.zeros(words, dtype=torch.int32, device=self.device)
            self._state_host = torch.zeros(words, dtype=torch.int32).pin_memory()

    def _warm_up(self) -> None:
        with torch.cuda.device(self.device), torch.no_grad():    # load every kernel of the ply before any capture
            self.reset()                                         # (a zeroed descriptor reserves no row: nothing is written)
            self._ply()
            self._ply()
        self.reset()

    _ws = property(lambda self: self.ply.ws)
    _ctl = property(lambda self: self.ply.ctl)

    def refresh(self) -> None:
        """After ``ppo.update()`` (or any in-place edit of weights): the group's snapshot follows the models."""
        self.group.refresh()

    def _fresh_seed(self) -> int:
        return self.seed if self.seed is not None else int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())

    # ------------------------------------------------------------------ chunks of plies
    def _capture(self, parity: int) -> torch.cuda.CUDAGraph:
        """Capture sync_every plies for the env's current buffer parity (an even count: the parity is the same afterwards)."""
        g = torch.cuda.CUDAGraph()
        # torch.cuda.graph does not collect garbage on entry.  Observed: a dead rollout object (captured graphs, pinned
        # buffers) still waiting in a reference cycle was collected inside a later capture, and the process aborted in its
        # destructor.  After a collection here, what the capture itself allocates holds no such object.
        gc.collect()
        with torch.cuda.graph(g):
            for _ in range(self.sync_every):
                self._ply()
        self._graphs[parity] = g
        return g

    def _chunk(self, plies: int) -> None:
        if self.graph and plies == self.sync_every:
            (self._graphs.get(self.env._cur) or self._capture(self.env._cur)).replay()
            return
        for _ in range(plies):
            self._ply_recorded() if self.record_enabled else self._ply()

    # ------------------------------------------------------------------ host side
    def _describe(self, buffer: KataGoRolloutBuffer, base: int, rows: int) -> dict:
        """Reserve ``rows`` rows behind the ones committed and point the kernel at the columns."""
        cols = buffer.reserve(rows, self.device, env_ids=self._ENV_IDS)
        d = self._desc_host
        for i, key in enumerate(_DESC_KEYS):
            d[i] = cols[key].data_ptr() if key in cols else 0
        d[12], d[13] = base, buffer._write_offset - base + rows
        self._desc.copy_(d, non_blocking=True)
        return cols

    def _read_state(self, stats) -> np.ndarray:
        """The one device -> host read of a sync point and its guards, in the reference's order and words.  It raises
        before the commit: a chunk with a guard fired is not kept."""
        name = type(self).__name__
        self._state_host.copy_(self._state)
        stats.host_syncs += 1
        st = self._state_host.numpy()
        self._zero_legal(st)
        if st[self._SAMP]:
            raise RuntimeError(f"NaN in raw policy logits in {name} — probability tensor contains nan "
                               f"({self._DIVERGED} has diverged)")
        if st[self._REFUSAL] or st[self._REFUSAL + 1]:
            self.env.raise_if_refused()
        self._protocol_guards(st)
        g = st[_GUARDS:_GUARDS + 4]
        peak = float(g[3:4].view(np.float32)[0])
        if g[:3].any() or peak > 3.5:                  # the rollout store's input guards, with the reference's messages
            _check_step_inputs(torch.tensor([not g[0]]), torch.tensor([True]), torch.tensor([5 if g[1] else 0]),
                               torch.tensor([float("nan") if g[2] else peak]))
        if st[_DROPPED] or st[_TRUNC_DROPPED]:
            raise RuntimeError(f"{name}: {int(st[_DROPPED])} rows did not fit the rows reserved in the rollout "
                               f"buffer, {int(st[_TRUNC_DROPPED])} truncations found no slot")
        return st

    def _protocol_guards(self, st: np.ndarray) -> None:
        """Guards of the subclass's own protocol, between the refusal latch and the store's input guards."""

    def _after_commit(self, st: np.ndarray, cols: dict, stats, dropped_before: int) -> None:
        """Behind a sync point's commit: the finished games leave the log, the truncated rows get their bootstrap."""
        if self.game_log is not None:
            stats.games += self.game_log.drain()
            stats.games_dropped = self.game_log.dropped - dropped_before
        n = int(st[_TRUNC])
        if n:
            self._overrides(cols, n)
            stats.truncation_overrides += n

    def _tallies(self, st: np.ndarray, stats) -> None:
        stats.rows = int(st[_ROWS])
        stats.wins, stats.losses, stats.draws = int(st[_WINS]), int(st[_LOSSES]), int(st[_DRAWS])
        stats.black_wins, stats.white_wins = int(st[_BLACK]), int(st[_WHITE])
        stats.terminated, stats.truncated = int(st[_TERMINATED]), int(st[_TRUNCATED])

    def _learner_values(self, obs: torch.Tensor, n: int, ws: Optional[dict]) -> torch.Tensor:
        _, vl, sc = self.group._tables.forward(obs, self._learner_of[:n], ws=ws)
        v = torch.empty(n, device=self.device)
        _lib.call("ka_scalar_value", vl, sc if self.alpha != 0.0 else None, self.alpha, v, n, _lib.stream_ptr(self.device))
        return v

    def _check_buffer(self, buffer, steps: int, num_envs: Optional[int] = None) -> None:
        if steps < 1:
            raise ValueError(f"steps must be positive, got {steps}")
        if not isinstance(buffer, KataGoRolloutBuffer):
            raise ValueError(f"collect() writes a KataGoRolloutBuffer, got {type(buffer).__name__}")
        if tuple(buffer.obs_shape) != _OBS_SHAPE or buffer.action_space != ACTION_SPACE:
            raise ValueError(f"buffer holds obs {tuple(buffer.obs_shape)} / {buffer.action_space} actions, the env gives "
                             f"{_OBS_SHAPE} / {ACTION_SPACE}")
        if num_envs is not None and buffer.num_envs != num_envs:
            raise ValueError(f"buffer is laid out for {buffer.num_envs} envs, the rollout steps {num_envs}")
        bd = buffer._device
        if bd is not None and (bd.type != "cuda" or (bd.index is not None and bd.index != self.device.index)):
            raise ValueError(f"buffer lives on {buffer._device}, the rollout on {self.device} (a device-resident buffer)")

    def _run_collect(self, buffer, steps: int, stats):
        with torch.cuda.device(self.device), torch.no_grad():
            self._collect(buffer, int(steps), stats)
        return stats
