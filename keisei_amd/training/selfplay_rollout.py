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

The front of the ply and the skeleton around it are ``_device_ply.py``'s (``DevicePly``, ``DeviceRollout``), shared with
``LeagueRollout``.  ``_selfplay_host`` restates the branch on the CPU from this package's host pieces (a host
``KataGoRolloutBuffer``, ``_compute_value_cats``, the tallies); the tests hold the kernel to it and hold it to the
reference (tests/golden/g14_selfplay_rollout.npz).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np
import torch

from keisei_amd import _lib
from keisei_amd.shogi_gym import MASK_WORDS

from ._device_ply import (_OBS_ELEMS, _DROPPED, _PLY, _ROWS, _SAMP, _SEED, _TRUNC, _TRUNC_DROPPED,  # noqa: F401
                          DeviceRollout, check_loop_args, check_value_args)
from .game_log import RecordedGame
from .katago_loop import _compute_value_cats
from .katago_ppo import SCORE_NORMALIZATION, KataGoRolloutBuffer
from .model_group import SEResNetGroup

__all__ = ["SelfPlayRollout", "SelfPlayStats"]

_PLIES, _STALL = 4, 25                  # state words of csrc/selfplay.hip beside the ones it shares with the league's
_ZERO_LEGAL = "Environments {envs} have zero legal actions — all-False legal mask would produce NaN"      # select_actions' text


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
                value_adapter, start_pool_capacity: int = 0, game_log: int = 0) -> None:
    if _lib.available():
        top = _lib.query("ka_selfplay_layout", 3)
        if not 1 <= num_envs <= top:
            raise ValueError(f"num_envs must lie in [1, {top}], got {num_envs}")
    elif num_envs < 1:
        raise ValueError(f"num_envs must be positive, got {num_envs}")
    check_loop_args(max_ply, sync_every, graph, record, start_pool_capacity, game_log, one_truncation_slot=True)
    check_value_args(score_norm, value_adapter)


class SelfPlayRollout(DeviceRollout):
    """The learner's self-play rollout, resident on the device (see module docstring).

    ``roll = SelfPlayRollout(learner, num_envs=512, max_ply=500, ...)``; ``stats = roll.collect(buffer, steps)`` steps
    every env ``steps`` plies and leaves ``steps x num_envs`` transitions in ``buffer`` (a device-resident
    ``KataGoRolloutBuffer`` in the dense layout; ``buffer.size`` grows by ``steps``); ``roll.bootstrap_values()`` is the
    ``next_values`` of ``KataGoPPOAlgorithm.update``; ``roll.refresh()`` after the update brings the learner's new weights
    into the group.  The env is not reset between ``collect`` calls (the reference carries games over epochs);
    ``reset()`` is explicit.  ``seed`` fixes sampling from the last ``reset()`` on.  ``record=True`` (no graph) keeps every
    ply's inputs and outputs in ``self.record`` for tests.  ``start_pool_capacity``, ``game_log``, ``move_history``,
    ``insight`` and ``insight_temperature`` are ``DevicePly``'s (``_device_ply.py``); here the log's launch is
    ``ka_gamelog_step``, ``collect`` drains it onto ``SelfPlayStats.games``, and every ``spectator_data()`` dict carries
    ``value_estimate``.  Without an option the ply is launch for launch what it is without it.
    There are no sampling controls here (``sampling.py``), on purpose: the single model is the learner, and its draws are
    the PPO behaviour policy."""

    _LAYOUT, _ENV_IDS, _DIVERGED = "ka_selfplay_layout", False, "the model"

    def __init__(self, learner, *, num_envs: int = 512, max_ply: int = 500, value_adapter=None,
                 score_norm: float = SCORE_NORMALIZATION, sync_every: int = 32, graph: bool = True,
                 seed: Optional[int] = None, record: bool = False, start_pool_capacity: int = 0,
                 game_log: int = 0, move_history: bool = False, insight: int = 0,
                 insight_temperature: float = 1.0) -> None:
        _check_args(int(num_envs), int(max_ply), int(sync_every), bool(graph), bool(record), float(score_norm), value_adapter,
                    start_pool_capacity, game_log)
        self.learner = learner
        self._build(self._make_group(learner), num_envs=num_envs, max_ply=max_ply, sync_every=sync_every, graph=graph,
                    seed=seed, record=record, value_adapter=value_adapter, score_norm=score_norm,
                    trunc_words=_lib.query("ka_selfplay_layout", 2), start_pool_capacity=int(start_pool_capacity),
                    game_log=game_log, move_history=move_history, insight=insight, insight_temperature=insight_temperature)
        self._new_state(_lib.query("ka_selfplay_state_words"))
        self._warm_up()

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

    # ------------------------------------------------------------------ state
    def reset(self) -> None:
        """Every env back to the start position, counters cleared, fresh seed."""
        seed = self._fresh_seed()
        with torch.cuda.device(self.device):
            hdr = torch.zeros(self._state.shape, dtype=torch.int32)
            hdr[_SEED:_SEED + 2].view(torch.int64)[0] = seed
            self._state.copy_(hdr)
            self._desc.zero_()
            self._stall.zero_()
            self._values.zero_()
            self.ply.reset()
        self.record = []

    @property
    def last_values(self) -> torch.Tensor:
        """The learner's value of every env at the last ply (the reference's ``latest_values``, :1446)."""
        return self._values

    # ------------------------------------------------------------------ one ply
    def _ply(self) -> None:
        """forward -> sample -> step -> bookkeeping on the current stream; no host synchronisation."""
        ply, N = self.ply, self.num_envs
        sp = self._state.data_ptr()
        cur, pre, value, score, st = ply.move(self._model_of, 1, sp, sp + 4 * self._SAMP)
        r = ply.step()
        ply.log(r, pre, ply_counter=sp + 4 * _PLIES)      # before ka_selfplay_step advances the ply counter it stamps
        _lib.call("ka_selfplay_step", self._state, N, cur.observations, cur.legal_mask_bits, self._actions, self._logp,
                  value, score if self.alpha != 0.0 else None, self.alpha, self._nlegal, pre, r.rewards,
                  r.terminated, r.truncated, r.step_metadata.material_balance, self.score_norm, r.terminal_observations,
                  self.env._err.data_ptr() + 8, self._stall, self._values, self._t_obs, self._t_list, self._desc, self._plan,
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

    # ------------------------------------------------------------------ host side
    def _zero_legal(self, st: np.ndarray) -> None:
        if st[_STALL] or st[self._SAMP + 1]:
            raise RuntimeError(_ZERO_LEGAL.format(envs=np.flatnonzero(self._stall.cpu().numpy()).tolist()))

    def _overrides(self, cols: dict, n: int) -> None:
        """The deferred truncation bootstrap (:1496-1521): one learner forward over the n parked terminal observations,
        negated into the mover's frame, scattered into the rows' next_value_override."""
        tl = self._t_list[:n]
        v = self._learner_values(self._t_obs[:n], n, None)
        cols["next_value_override"].index_copy_(0, tl[:, 1].long(), -v)
        self._state[_TRUNC:_TRUNC + 1].zero_()

    def collect(self, buffer: KataGoRolloutBuffer, steps: int) -> SelfPlayStats:
        """Step every env ``steps`` plies; ply p's transitions are rows [p * N, (p + 1) * N) behind the buffer's rows."""
        self._check_buffer(buffer, steps, self.num_envs)
        if buffer._write_offset and buffer._has_env_ids:
            raise ValueError("buffer already holds rows in the env_ids layout (split-merge / LeagueRollout); SelfPlayRollout "
                             "writes the dense (T, N) layout without env_ids: clear() the buffer or use another one")
        return self._run_collect(buffer, steps, SelfPlayStats())

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
            self._after_commit(st, cols, stats, dropped_before)
            done += plies
        buffer.fill_alternating_perspective_overrides()            # :1590; fills NaN cells of non-terminal rows only
        stats.plies = steps
        self._tallies(st, stats)

    def live_games(self, envs: Optional[Sequence[int]] = None) -> List[RecordedGame]:
        """The games in progress (every env, or ``envs``) between two ``collect`` calls: ``RecordedGame`` with
        ``finished=False``."""
        return self.ply.live_games("a rollout", envs, ply_counter=self._state.data_ptr() + 4 * _PLIES)

    def spectator_data(self, envs: Optional[Sequence[int]] = None) -> List[dict]:
        """``DevicePly.spectator_data`` between two ``collect`` calls, each dict with ``value_estimate``: the learner's
        value at the env's last ply (the reference's snapshot row takes it from ``latest_values``,
        katago_loop.py:1938-1942)."""
        return self.ply.spectator_data(envs, self._values)

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
