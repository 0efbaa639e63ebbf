"""SelfPlayRollout: the self-play rollout epoch on the device (the no-opponent branch of the reference's
``KataGoTrainingLoop.run``, katago_loop.py:1438-1527, and the bootstrap behind it, :1565-1590).

No opponent is seated: every env is the learner and every ply gives one transition per env.  The learner sits alone in
``SEResNetGroup([learner])`` (its forward in this loop is an eval-mode, no-grad forward, katago_ppo.py:553).  One ply is
four steps on one stream, with no host synchronisation:

    grouped stem / tower / heads, every row model 0   (csrc/tower.hip, the group's tables)
    ka_policy_sample_play, K = 1                        (csrc/loss.hip: actions and log-probs, seed read from the device)
    ka_shogi_env_step                                   (csrc/shogi_env.hip)
    ka_gamelog_step                                     (csrc/gamelog.hip, only with game_log > 0: the finished games, move by move)
    ka_selfplay_step                                    (csrc/selfplay.hip: tallies, the env's row straight into the rollout
                                                         store's columns, input guards, truncation slots)

``sync_every`` plies are captured as one graph per ``VecEnv`` buffer parity; the host reads ONE state array per chunk.
Env e at ply p of a ``collect`` owns row ``base + p * N + e`` of a device-resident ``KataGoRolloutBuffer`` reserved with
``env_ids=False``: the dense (T, N) layout of the reference's ``add()`` calls in this branch.  The kernel reads the column
pointers from a small device descriptor the host rewrites at each sync point, so a captured graph survives a store
that grows.  The bootstrap override of truncated games (:1496-1521) is deferred: the kernel parks the terminal
observation, the host runs one learner forward over exactly those rows at the sync point and writes ``-V``.  The
learner's weights do not change inside ``collect`` and eval mode couples no two boards, so the values are what an in-ply
forward gives.

``_selfplay_host`` restates the branch on the CPU from this package's host pieces (a host ``KataGoRolloutBuffer``,
``_compute_value_cats``, the tallies); the tests hold the kernel to it and hold it to the reference
(tests/golden/g14_selfplay_rollout.npz).
"""
from __future__ import annotations

import gc
import math
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from keisei_amd import _lib
from keisei_amd.shogi_gym import ACTION_SPACE, MASK_WORDS, OBS_CHANNELS, VecEnv

from .game_log import GameLog, RecordedGame
from .katago_loop import _compute_value_cats
from .katago_ppo import SCORE_NORMALIZATION, KataGoRolloutBuffer, _check_step_inputs
from .model_group import SEResNetGroup
from .policy_insight import InsightRecorder
from .value_adapter import MultiHeadValueAdapter

__all__ = ["SelfPlayRollout", "SelfPlayStats"]

_OBS_SHAPE = (OBS_CHANNELS, 9, 9)
_OBS_ELEMS = OBS_CHANNELS * 81
# state words (csrc/selfplay.hip)
_SEED, _PLY, _ROWS, _PLIES, _DROPPED, _SAMP, _REFUSAL, _TRUNC, _TRUNC_DROPPED = 0, 2, 3, 4, 5, 6, 8, 12, 13
_WINS, _LOSSES, _DRAWS, _BLACK, _WHITE, _TERMINATED, _TRUNCATED, _GUARDS, _STALL = 14, 15, 16, 17, 18, 19, 20, 21, 25
_ZERO_LEGAL = "Environments {envs} have zero legal actions — all-False legal mask would produce NaN"      # select_actions' text
_DESC_KEYS = ("observations", "legal_masks", "actions", "log_probs", "values", "rewards", "dones", "terminated",
              "value_categories", "score_targets", "env_ids", "next_value_override")


@dataclass
class SelfPlayStats:
    plies: int = 0
    rows: int = 0                       # transitions written to the buffer: plies x envs
    wins: int = 0                       # terminated games, the mover's frame
    losses: int = 0
    draws: int = 0
    black_wins: int = 0
    white_wins: int = 0
    terminated: int = 0
    truncated: int = 0                  # truncated and not terminated
    host_syncs: int = 0                 # reads of the state array
    truncation_overrides: int = 0       # rows whose bootstrap override was computed at a sync point
    games: List[RecordedGame] = field(default_factory=list)     # the finished games (a rollout built with game_log > 0)
    games_dropped: int = 0              # finished games that did not fit the log between two sync points


def _check_args(num_envs: int, max_ply: int, sync_every: int, graph: bool, record: bool, score_norm: float,
                value_adapter) -> None:
    if _lib.available():
        top = _lib.query("ka_selfplay_layout", 3)
        if not 1 <= num_envs <= top:
            raise ValueError(f"num_envs must lie in [1, {top}], got {num_envs}")
    elif num_envs < 1:
        raise ValueError(f"num_envs must be positive, got {num_envs}")
    if not 1 <= max_ply <= 65535:
        raise ValueError(f"max_ply must lie in [1, 65535], got {max_ply}")
    if sync_every < 1:
        raise ValueError(f"sync_every must be at least 1, got {sync_every}")
    if sync_every > max_ply:
        raise ValueError(f"sync_every ({sync_every}) must not exceed max_ply ({max_ply}): an env may truncate only once "
                         "between two sync points (one truncation slot per env)")
    if graph and record:
        raise ValueError("record=True runs without a graph (graph=False)")
    if graph and sync_every % 2:
        raise ValueError(f"graph=True needs an even sync_every (VecEnv alternates two result buffers), got {sync_every}")
    if not math.isfinite(score_norm) or score_norm == 0:
        raise ValueError(f"score_norm must be finite and non-zero, got {score_norm}")
    if value_adapter is not None and type(value_adapter) is not MultiHeadValueAdapter:
        raise ValueError(f"value_adapter must be None or a MultiHeadValueAdapter (the kernel blends by its "
                         f"score_blend_alpha), got {type(value_adapter).__name__}")


class SelfPlayRollout:
    """The learner's self-play rollout, resident on the device (see module docstring).

    ``roll = SelfPlayRollout(learner, num_envs=512, max_ply=500, ...)``; ``stats = roll.collect(buffer, steps)`` steps
    every env ``steps`` plies and leaves ``steps x num_envs`` transitions in ``buffer`` (a device-resident
    ``KataGoRolloutBuffer`` in the dense layout; ``buffer.size`` grows by ``steps``); ``roll.bootstrap_values()`` is the
    ``next_values`` of ``KataGoPPOAlgorithm.update``; ``roll.refresh()`` after the update brings the learner's new weights
    into the group.  The env is not reset between ``collect`` calls (the reference carries games over epochs);
    ``reset()`` is explicit.  ``seed`` fixes sampling from the last ``reset()`` on.  ``record=True`` (no graph) keeps every
    ply's inputs and outputs in ``self.record`` for tests.  ``start_pool_capacity > 0`` gives the env a pool of
    start positions of that size: ``roll.env.set_start_positions(...)`` / ``set_start_sfens(...)`` between ``collect`` calls make later
    games start from them (no re-capture; see ``VecEnv``).  ``game_log=K > 0`` adds a device-resident ``GameLog`` of K
    records to the ply (one launch, ``ka_gamelog_step``, between the env step and ``ka_selfplay_step``): ``collect``
    drains it at every sync point onto ``SelfPlayStats.games``.  Without it the ply is launch for launch what it was.
    ``move_history=True`` has the env keep the move notes of the games in progress (two more launches inside ``env.step``,
    see ``VecEnv``); ``spectator_data()`` between two ``collect`` calls is the dashboard feed either way.
    ``insight=top_k > 0`` adds the policy insight to the ply (one launch, ``ka_policy_insight``, between the sampler and the
    env step; ``policy_insight.py``): every ``spectator_data()`` dict gains ``insight``, the figures of the env's last move at
    ``insight_temperature``, and with ``move_history=True`` every history entry gains its move's probability, rank, entropy,
    win probability and top candidates.  With 0 the ply and every dict are what they were.
    There are no sampling controls here (``sampling.py``), on purpose: the single model is the learner, and its draws are
    the PPO behaviour policy."""

    def __init__(self, learner, *, num_envs: int = 512, max_ply: int = 500, value_adapter=None,
                 score_norm: float = SCORE_NORMALIZATION, sync_every: int = 32, graph: bool = True,
                 seed: Optional[int] = None, record: bool = False, start_pool_capacity: int = 0,
                 game_log: int = 0, move_history: bool = False, insight: int = 0,
                 insight_temperature: float = 1.0) -> None:
        _check_args(int(num_envs), int(max_ply), int(sync_every), bool(graph), bool(record), float(score_norm), value_adapter)
        if start_pool_capacity < 0:
            raise ValueError(f"start_pool_capacity must not be negative, got {start_pool_capacity}")
        if game_log < 0:
            raise ValueError(f"game_log must not be negative, got {game_log}")
        self.group = self._make_group(learner)
        self.learner = learner
        self.device = self.group.device
        self.num_envs, self.max_ply, self.sync_every = int(num_envs), int(max_ply), int(sync_every)
        self.graph, self.seed, self.record_enabled = bool(graph), seed, bool(record)
        self.value_adapter, self.score_norm = value_adapter, float(score_norm)
        self.alpha = 0.0 if value_adapter is None else float(value_adapter.score_blend_alpha)
        self.record: List[dict] = []
        N, dev = self.num_envs, self.device
        q = lambda which: _lib.query("ka_selfplay_layout", which)  # noqa: E731
        with torch.cuda.device(dev):
            z = lambda *s, dtype=torch.int32: torch.zeros(*s, dtype=dtype, device=dev)  # noqa: E731
            self.env = VecEnv(N, self.max_ply, "katago", "spatial", device=dev, output="torch", check_actions=False,
                              start_pool_capacity=int(start_pool_capacity), move_history=bool(move_history))
            self._actions, self._logp, self._nlegal = z(N, dtype=torch.int64), z(N, dtype=torch.float32), z(N)
            self._values = z(N, dtype=torch.float32)
            self._model_of = z(N)                                    # every row on model 0
            self._stall = z(N, dtype=torch.uint8)
            self._t_obs, self._t_list = z(N, *_OBS_SHAPE, dtype=torch.float32), z(N, q(2))
            self._plan = z(N, q(0))
            self._desc = z(q(1), dtype=torch.int64)
            self._desc_host = torch.zeros(q(1), dtype=torch.int64).pin_memory()
            self._state = z(_lib.query("ka_selfplay_state_words"))
            self._state_host = torch.zeros(self._state.shape, dtype=torch.int32).pin_memory()
            self._ws = self.group._tables.workspace(N)
            self.game_log: Optional[GameLog] = GameLog(self.env, capacity=int(game_log)) if game_log else None
            self.insight: Optional[InsightRecorder] = InsightRecorder(self.env, insight, insight_temperature) if insight else None
        self._graphs: Dict[int, torch.cuda.CUDAGraph] = {}
        with torch.cuda.device(dev), torch.no_grad():            # load every kernel of the ply before any capture
            self.reset()                                         # (a zeroed descriptor reserves no row: nothing is written)
            self._ply()
            self._ply()
        self.reset()

    @staticmethod
    def _make_group(learner) -> SEResNetGroup:
        try:
            group = SEResNetGroup([learner])
        except ValueError as e:
            raise ValueError(f"SelfPlayRollout needs the learner as an SEResNetModel of a shape the group covers, on a "
                             f"GPU ({e}); use select_actions' loop for this model") from e
        if group.device.type != "cuda" or group._tables is None:
            raise ValueError(f"SelfPlayRollout runs on a GPU group; this model is on {group.device}: use select_actions' "
                             "loop for this model")
        return group

    def refresh(self) -> None:
        """After ``ppo.update()`` (or any in-place edit of weights): the group's snapshot follows the model."""
        self.group.refresh()

    # ------------------------------------------------------------------ state
    def reset(self) -> None:
        """Every env back to the start position, counters cleared, fresh seed."""
        seed = self.seed if self.seed is not None else int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        with torch.cuda.device(self.device):
            hdr = torch.zeros(self._state.shape, dtype=torch.int32)
            hdr[_SEED:_SEED + 2].view(torch.int64)[0] = seed
            self._state.copy_(hdr)
            self._desc.zero_()
            self._stall.zero_()
            self._values.zero_()
            self.env.reset()
            if self.game_log is not None:
                self.game_log.begin()
            if self.insight is not None:
                self.insight.clear()
        self.record = []

    @property
    def last_values(self) -> torch.Tensor:
        """The learner's value of every env at the last ply (the reference's ``latest_values``, :1446)."""
        return self._values

    # ------------------------------------------------------------------ one ply
    def _ply(self) -> None:
        """forward -> sample -> step -> bookkeeping on the current stream; no host synchronisation."""
        env, N = self.env, self.num_envs
        st = _lib.stream_ptr(self.device)
        cur, prev = env.current(), env._cur
        logits, value, score = self.group._tables.forward(cur.observations, self._model_of, ws=self._ws)
        sp = self._state.data_ptr()
        _lib.call("ka_policy_sample_play", logits, 0, cur.legal_mask_bits, MASK_WORDS, sp, self._model_of, 1,
                  self._actions, self._logp, self._nlegal, sp + 4 * _SAMP, N, ACTION_SPACE, st)
        if self.insight is not None:                      # while the logits exist, before the step moves the history count
            self.insight.step(logits, cur.legal_mask_bits, self._actions, value, env._players[prev], self._model_of, 1,
                              sp + 4 * _SAMP, st)
        r = env.step(self._actions)
        if self.game_log is not None:                     # before ka_selfplay_step advances the ply counter it stamps
            self.game_log.step(self._actions, r.rewards, r.terminated, r.truncated, env._players[prev],
                               r.step_metadata.termination_reason, nlegal=self._nlegal, ply_counter=sp + 4 * _PLIES)
        _lib.call("ka_selfplay_step", self._state, N, cur.observations, cur.legal_mask_bits, self._actions, self._logp,
                  value, score if self.alpha != 0.0 else None, self.alpha, self._nlegal, env._players[prev], r.rewards,
                  r.terminated, r.truncated, r.step_metadata.material_balance, self.score_norm, r.terminal_observations,
                  env._err.data_ptr() + 8, self._stall, self._values, self._t_obs, self._t_list, self._desc, self._plan,
                  _OBS_ELEMS, MASK_WORDS, st)

    def _ply_recorded(self) -> None:
        env = self.env
        cur, prev = env.current(), env._cur
        rec = {"seed": int(self._state[:2].view(torch.int64).item()), "obs": cur.observations.cpu(),
               "mask_bits": cur.legal_mask_bits.cpu(), "pre_players": env._players[prev].cpu().numpy()}
        self._ply()
        c = env._cur
        trunc = (env._truncated[c] & ~env._terminated[c]).nonzero(as_tuple=True)[0]
        rec.update(actions=self._actions.cpu().numpy(), log_probs=self._logp.cpu().numpy(), values=self._values.cpu().numpy(),
                   n_legal=self._nlegal.cpu().numpy(), rewards=env._rewards[c].cpu().numpy(),
                   terminated=env._terminated[c].cpu().numpy(), truncated=env._truncated[c].cpu().numpy(),
                   current_players=env._players[c].cpu().numpy(), material=env._material[c].cpu().numpy(),
                   terminal_envs=trunc.cpu().numpy(), terminal_obs=env._terminal_obs[trunc].cpu())
        self.record.append(rec)

    def _capture(self, parity: int) -> torch.cuda.CUDAGraph:
        """Capture sync_every plies for the env's current buffer parity (an even count: the parity is the same afterwards)."""
        g = torch.cuda.CUDAGraph()
        # torch.cuda.graph does not collect garbage on entry: a dead rollout object (captured graphs, pinned buffers) still
        # waiting in a reference cycle must not be collected inside the capture (see LeagueRollout._capture)
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
        """Reserve ``rows`` dense rows behind the ones committed and point the kernel at the columns."""
        cols = buffer.reserve(rows, self.device, env_ids=False)
        d = self._desc_host
        for i, key in enumerate(_DESC_KEYS):
            d[i] = cols[key].data_ptr() if key in cols else 0
        d[12], d[13] = base, buffer._write_offset - base + rows
        self._desc.copy_(d, non_blocking=True)
        return cols

    def _read_state(self, stats: SelfPlayStats) -> np.ndarray:
        self._state_host.copy_(self._state)           # the one device -> host read of a sync point
        stats.host_syncs += 1
        st = self._state_host.numpy()
        if st[_STALL] or st[_SAMP + 1]:
            raise RuntimeError(_ZERO_LEGAL.format(envs=np.flatnonzero(self._stall.cpu().numpy()).tolist()))
        if st[_SAMP]:
            raise RuntimeError("NaN in raw policy logits in SelfPlayRollout — probability tensor contains nan "
                               "(the model has diverged)")
        if st[_REFUSAL] or st[_REFUSAL + 1]:
            self.env.raise_if_refused()
        g = st[_GUARDS:_GUARDS + 4]
        peak = float(g[3:4].view(np.float32)[0])
        if g[:3].any() or peak > 3.5:                  # the rollout store's input guards, with the reference's messages
            _check_step_inputs(torch.tensor([not g[0]]), torch.tensor([True]), torch.tensor([5 if g[1] else 0]),
                               torch.tensor([float("nan") if g[2] else peak]))
        if st[_DROPPED] or st[_TRUNC_DROPPED]:
            raise RuntimeError(f"SelfPlayRollout: {int(st[_DROPPED])} rows did not fit the rows reserved in the rollout "
                               f"buffer, {int(st[_TRUNC_DROPPED])} truncations found no slot")
        return st

    def _overrides(self, cols: dict, n: int) -> None:
        """The deferred truncation bootstrap (:1496-1521): one learner forward over the n parked terminal observations,
        negated into the mover's frame, scattered into the rows' next_value_override."""
        tl = self._t_list[:n]
        v = self._learner_values(self._t_obs[:n], n, None)
        cols["next_value_override"].index_copy_(0, tl[:, 1].long(), -v)
        self._state[_TRUNC:_TRUNC + 1].zero_()

    def _learner_values(self, obs: torch.Tensor, n: int, ws: Optional[dict]) -> torch.Tensor:
        _, vl, sc = self.group._tables.forward(obs, self._model_of[:n], ws=ws)
        v = torch.empty(n, device=self.device)
        _lib.call("ka_scalar_value", vl, sc if self.alpha != 0.0 else None, self.alpha, v, n, _lib.stream_ptr(self.device))
        return v

    def collect(self, buffer: KataGoRolloutBuffer, steps: int) -> SelfPlayStats:
        """Step every env ``steps`` plies; ply p's transitions are rows [p * N, (p + 1) * N) behind the buffer's rows."""
        if steps < 1:
            raise ValueError(f"steps must be positive, got {steps}")
        if not isinstance(buffer, KataGoRolloutBuffer):
            raise ValueError(f"collect() writes a KataGoRolloutBuffer, got {type(buffer).__name__}")
        if tuple(buffer.obs_shape) != _OBS_SHAPE or buffer.action_space != ACTION_SPACE:
            raise ValueError(f"buffer holds obs {tuple(buffer.obs_shape)} / {buffer.action_space} actions, the env gives "
                             f"{_OBS_SHAPE} / {ACTION_SPACE}")
        if buffer.num_envs != self.num_envs:
            raise ValueError(f"buffer is laid out for {buffer.num_envs} envs, the rollout steps {self.num_envs}")
        bd = buffer._device
        if bd is not None and (bd.type != "cuda" or (bd.index is not None and bd.index != self.device.index)):
            raise ValueError(f"buffer lives on {buffer._device}, the rollout on {self.device} (a device-resident buffer)")
        if buffer._write_offset and buffer._has_env_ids:
            raise ValueError("buffer already holds rows in the env_ids layout (split-merge / LeagueRollout); SelfPlayRollout "
                             "writes the dense (T, N) layout without env_ids: clear() the buffer or use another one")
        stats = SelfPlayStats()
        with torch.cuda.device(self.device), torch.no_grad():
            self._collect(buffer, int(steps), stats)
        return stats

    def _collect(self, buffer, steps, stats) -> None:
        N = self.num_envs
        self.record = []
        self._state[_PLY:_ROWS + 1].zero_()
        self._state[_DROPPED:_SAMP + 2].zero_()
        self._state[_TRUNC:].zero_()
        self._stall.zero_()
        base, done, st = buffer._write_offset, 0, None
        dropped_before = self.game_log.dropped if self.game_log is not None else 0
        while done < steps:
            plies = min(self.sync_every, steps - done)
            cols = self._describe(buffer, base, plies * N)
            self._chunk(plies)
            st = self._read_state(stats)               # raises before the commit: a chunk with a guard fired is not kept
            buffer.commit(plies * N, plies)
            if self.game_log is not None:
                stats.games += self.game_log.drain()
                stats.games_dropped = self.game_log.dropped - dropped_before
            n = int(st[_TRUNC])
            if n:
                self._overrides(cols, n)
                stats.truncation_overrides += n
            done += plies
        buffer.fill_alternating_perspective_overrides()            # :1590; fills NaN cells of non-terminal rows only
        stats.plies, stats.rows = steps, int(st[_ROWS])
        stats.wins, stats.losses, stats.draws = int(st[_WINS]), int(st[_LOSSES]), int(st[_DRAWS])
        stats.black_wins, stats.white_wins = int(st[_BLACK]), int(st[_WHITE])
        stats.terminated, stats.truncated = int(st[_TERMINATED]), int(st[_TRUNCATED])

    def live_games(self, envs: Optional[Sequence[int]] = None) -> List[RecordedGame]:
        """The games in progress (every env, or ``envs``) between two ``collect`` calls: ``RecordedGame`` with
        ``finished=False``."""
        if self.game_log is None:
            raise ValueError("live_games() needs a rollout built with game_log > 0")
        with torch.cuda.device(self.device):
            return self.game_log.live(envs, ply_counter=self._state.data_ptr() + 4 * _PLIES)

    def spectator_data(self, envs: Optional[Sequence[int]] = None) -> List[dict]:
        """``VecEnv.get_spectator_data`` of every env (or ``envs``) between two ``collect`` calls, each dict with
        ``value_estimate``: the learner's value at the env's last ply (the reference's snapshot row takes it from
        ``latest_values``, katago_loop.py:1938-1942).  ``move_history`` is [] unless built with ``move_history=True``;
        ``insight`` (built with ``insight > 0``) is the ``insight_dict`` of the env's last move, None before its first move
        after ``reset()``."""
        with torch.cuda.device(self.device):
            data = self.env.get_spectator_data(envs)
            values = self._values.cpu().numpy()
        ids = range(self.num_envs) if envs is None else [int(e) for e in envs]
        for d, e in zip(data, ids):
            d["value_estimate"] = float(values[e])
        if self.insight is not None:
            with torch.cuda.device(self.device):
                self.insight.annotate(data, envs)
        return data

    def bootstrap_values(self) -> torch.Tensor:
        """-V(observation now) by the learner (katago_loop.py:1565-1572, :1589): ``update``'s next_values, in the frame of
        the last ply's mover."""
        with torch.cuda.device(self.device), torch.no_grad():
            return -self._learner_values(self.env.current().observations, self.num_envs, self._ws)


# ---------------------------------------------------------------------------------------------- host restatement
def _truncated_only(terminated: torch.Tensor, truncated: torch.Tensor) -> torch.Tensor:
    """:1502 -- the envs whose game was cut short, not decided."""
    return truncated & ~terminated


def _override_of(term_values: torch.Tensor) -> torch.Tensor:
    """:1521 -- the terminal observation speaks for the side to move, GAE wants the mover of the step."""
    return -term_values


def _selfplay_host(records: Sequence[dict], *, num_envs: int, obs_shape: tuple, action_space: int, score_norm: float,
                   final_values=None, prior: Optional[KataGoRolloutBuffer] = None, fill: bool = True):
    """The reference's no-opponent branch (katago_loop.py:1453-1527, :1589-1590) over per-ply records, on the CPU, from this
    package's host pieces.  A record holds one ply as arrays over all envs: ``obs``, ``mask_bits`` (packed int32 rows) or
    ``legal_masks`` (bool), ``pre_players``, ``actions``, ``log_probs``, ``values``, ``rewards``, ``terminated``,
    ``truncated``, ``material`` and, for plies with truncations, ``term_values`` (the learner's value of every env's
    terminal observation, before the negation; NaN where there is none).  ``final_values``: the learner's value of the
    observations behind the last record.  ``prior``: a host buffer to go on from (a second ``collect``).  ``fill=False``
    leaves out the alternating fill of :1590 (what ``ka_selfplay_step`` alone writes).
    Returns ``(columns, stats)``: the host buffer's ``flatten()`` after ``fill_alternating_perspective_overrides()`` plus
    ``size`` and, given ``final_values``, ``next_values``; the tallies as a dict."""
    t = lambda x, dt=None: torch.as_tensor(np.asarray(x), dtype=dt)  # noqa: E731
    dev = torch.device("cpu")
    buffer = prior if prior is not None else KataGoRolloutBuffer(num_envs, tuple(obs_shape), action_space)
    tally = dict(wins=0, losses=0, draws=0, black_wins=0, white_wins=0, terminated=0, truncated=0, truncation_overrides=0)
    for rec in records:
        rewards = t(rec["rewards"], torch.float32)
        terminated, truncated = t(rec["terminated"]).bool(), t(rec["truncated"]).bool()
        dones = terminated | truncated                           # :1458
        tally["terminated"] += int(terminated.sum())             # :1460-1461
        tally["truncated"] += int((truncated & ~terminated).sum())
        if terminated.any():                                     # :1463-1485
            tr = rewards[terminated]
            tally["wins"] += int((tr > 0).sum()); tally["losses"] += int((tr < 0).sum()); tally["draws"] += int((tr == 0).sum())
            who = t(rec["pre_players"]).to(torch.int64)[terminated]
            tally["black_wins"] += int((((tr > 0) & (who == 0)) | ((tr < 0) & (who == 1))).sum())
            tally["white_wins"] += int((((tr > 0) & (who == 1)) | ((tr < 0) & (who == 0))).sum())
        cats = _compute_value_cats(rewards, terminated, dev)     # :1487
        score_targets = t(rec["material"]).to(torch.float32) / score_norm      # :1491-1494
        trunc_only = _truncated_only(terminated, truncated)      # :1502
        override = None
        if bool(trunc_only.any()):                               # :1504-1521
            term_v = t(rec["term_values"], torch.float32)
            override = torch.full_like(term_v, float("nan"))
            override[trunc_only] = _override_of(term_v)[trunc_only]
            tally["truncation_overrides"] += int(trunc_only.sum())
        if "mask_bits" in rec:
            bits = np.asarray(rec["mask_bits"]).astype(np.int32).view(np.uint32)
            masks = t(((bits[:, np.arange(action_space) >> 5] >> (np.arange(action_space) & 31).astype(np.uint32)) & 1) != 0)
        else:
            masks = t(rec["legal_masks"]).bool()
        buffer.add(t(rec["obs"], torch.float32), t(rec["actions"], torch.long), t(rec["log_probs"], torch.float32),
                   t(rec["values"], torch.float32), rewards, dones, terminated, masks, cats, score_targets,
                   next_value_override=override)                 # :1523-1527
    if fill:
        buffer.fill_alternating_perspective_overrides()          # :1590
    cols = dict(buffer.flatten()) if buffer.size else {}
    cols["size"] = buffer.size
    if final_values is not None:
        cols["next_values"] = -t(final_values, torch.float32)    # :1589
    stats = dict(tally, plies=len(records), rows=buffer._write_offset)
    return cols, stats
