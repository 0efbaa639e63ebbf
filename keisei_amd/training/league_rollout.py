"""LeagueRollout: the learner-vs-league rollout epoch on the device (the opponent branch of the reference's
``KataGoTrainingLoop.run``, katago_loop.py:1162-1437, and the flush and bootstrap behind it, :1537-1580).

The learner and its cohort of opponents sit in one ``SEResNetGroup`` (learner = model 0, opponent k = model k + 1): the
learner's forward in this loop is an eval-mode, no-grad forward (katago_loop.py:333-343), so it can be seated like any
opponent.  One ply is four steps (five with a game log) on one stream, with no host synchronisation:

    grouped stem / tower / heads on model_of   (csrc/tower.hip, the group's tables)
    ka_policy_sample_play                       (csrc/loss.hip: actions and log-probs, seed read from the device)
    ka_shogi_env_step                           (csrc/shogi_env.hip)
    ka_gamelog_step_env                         (csrc/gamelog.hip, only with game_log > 0: the finished games, move by
                                                 move, with the learner's colour and the players' ids)
    ka_league_step                              (csrc/league.hip: the reference's whole per-step bookkeeping -- learner-frame
                                                 rewards and tallies, pending accumulate / settle / open / immediate
                                                 settle straight into the rollout store's columns, per-opponent results,
                                                 opponent and colour re-draws, the next model_of)

``sync_every`` plies are captured as one graph; the host reads ONE state array per chunk.  Nothing inside an epoch needs
a host decision, so a chunk's result does not depend on ``sync_every`` or on graph capture: the re-draws are a stateless
function of (seed, env, games that env has finished), restated in numpy below (``league_draw``).

Rows go straight into a device-resident ``KataGoRolloutBuffer`` (``reserve`` / ``commit``): the kernel reads the column
pointers from a small device descriptor the host rewrites at each sync point, so the captured graph survives a store
that grows.  The bootstrap override of truncated games (:1250-1283) is deferred: the kernel parks the terminal
observation, the host runs one learner forward over exactly those rows at the sync point.  The learner's weights do
not change inside ``collect`` and eval mode couples no two boards, so the values are what an in-ply forward gives.

The front of the ply and the skeleton around it are ``_device_ply.py``'s (``DevicePly``, ``DeviceRollout``), shared with
``SelfPlayRollout``.  ``_league_host`` restates the protocol on the CPU from this package's host pieces
(``PendingTransitions``, ``to_learner_perspective``, ``_compute_value_cats``, a host ``KataGoRolloutBuffer``); the tests
hold the kernel to it and hold it to the reference (tests/golden/g13_league_rollout.npz).
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from keisei_amd import _lib
from keisei_amd.shogi_gym import MASK_WORDS, POOL_ROW_BYTES

from ._device_ply import (_OBS_ELEMS, _OBS_SHAPE, _DROPPED, _PLY, _ROWS, _SAMP, _SEED, _TRUNC, _TRUNC_DROPPED,  # noqa: F401
                          DeviceRollout, check_loop_args, check_value_args)
from .game_log import RecordedGame
from .katago_loop import (_ZERO_LEGAL, PendingTransitions, _compute_value_cats, sign_correct_bootstrap,
                          to_learner_perspective)
from .katago_ppo import SCORE_NORMALIZATION, KataGoRolloutBuffer
from .model_group import SEResNetGroup
from .sampling import GAME_PLY_BYTE, SamplingControls, league_controls

__all__ = ["LeagueRollout", "LeagueRolloutStats", "league_draw", "draw_opponents", "draw_sides", "cum_thresholds"]

# state words of csrc/league.hip beside the ones it shares with the self-play kernel; _HDR: the per-opponent results begin
_BLOCKS, _DRAW_SEED, _CONFLICT, _STALL, _HDR = 4, 10, 25, 26, 32
SALT_OPPONENT, SALT_SIDE, SALT_EPOCH_SIDE = 0x6F70706F, 0x73696465, 0x65706F63


# ---------------------------------------------------------------------------------------------- draws (numpy form)
def _mix(x: np.ndarray) -> np.ndarray:
    """splitmix64 finaliser on uint64 arrays (wrapping arithmetic), as ``ka_mix64`` of csrc/common.h."""
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


def league_draw(seed: int, salt: int, env, n) -> np.ndarray:
    """h(salt, env, n) = mix(seed ^ mix((env << 32 | n) + salt)) as uint64: the draw of env ``env`` after its n-th
    finished game (include/keisei_amd.h, league rollout)."""
    env = np.asarray(env, dtype=np.uint64)
    n = np.asarray(n, dtype=np.uint64) & np.uint64(0xFFFFFFFF)
    with np.errstate(over="ignore"):
        key = ((env << np.uint64(32)) | n) + np.uint64(salt)
    return _mix(np.uint64(seed & (2 ** 64 - 1)) ^ _mix(key))


def cum_thresholds(weights: Optional[Sequence[float]], K: int) -> np.ndarray:
    """K uint32 thresholds of the cumulative opponent weights (uniform when None) on the 31-bit scale of the draw:
    opponent = first k with u < cum[k], u = h >> 33 < 2^31 = the threshold of the last opponent with a weight."""
    w = np.ones(K, dtype=np.float64) if weights is None else np.asarray(weights, dtype=np.float64).reshape(-1)
    if w.shape[0] != K:
        raise ValueError(f"opponent_weights holds {w.shape[0]} weights for {K} opponents")
    if not np.isfinite(w).all() or (w < 0).any() or w.sum() <= 0:
        raise ValueError("opponent_weights must be finite, non-negative and not all zero")
    cum = np.minimum(np.floor(np.cumsum(w) / w.sum() * 2.0 ** 31), 2.0 ** 31).astype(np.uint32)
    cum[int(np.flatnonzero(w > 0)[-1]):] = np.uint32(1 << 31)
    return cum


def draw_opponents(seed: int, env, n, cum: np.ndarray) -> np.ndarray:
    u = (league_draw(seed, SALT_OPPONENT, env, n) >> np.uint64(33)).astype(np.uint32)
    k = np.searchsorted(cum, u, side="right")                  # first k with u < cum[k]
    return np.minimum(k, len(cum) - 1).astype(np.int32)


def draw_sides(seed: int, env, n, salt: int = SALT_SIDE) -> np.ndarray:
    return (league_draw(seed, salt, env, n) >> np.uint64(63)).astype(np.uint8)


# ---------------------------------------------------------------------------------------------- stats
@dataclass
class LeagueRolloutStats:
    plies: int = 0
    rows: int = 0                       # transitions written to the buffer
    adds: int = 0                       # non-empty blocks: what the reference's sequence of add() calls counts
    wins: int = 0                       # terminated games, learner's frame
    losses: int = 0
    draws: int = 0
    black_wins: int = 0
    white_wins: int = 0
    terminated: int = 0
    truncated: int = 0                  # truncated and not terminated
    opponent_results: Dict[int, List[int]] = field(default_factory=dict)      # opponent id -> [wins, losses, draws]
    host_syncs: int = 0                 # reads of the state array
    truncation_overrides: int = 0       # rows whose bootstrap override was computed at a sync point
    flushed: int = 0                    # rows the flush at the end of collect closed (done = 0)
    games: List[RecordedGame] = field(default_factory=list)     # the finished games (a rollout built with game_log > 0)
    games_dropped: int = 0              # finished games that did not fit the log between two sync points


def _check_args(num_opponents: int, opponent_ids, num_envs: int, max_ply: int, sync_every: int, graph: bool, record: bool,
                score_norm: float, value_adapter, start_pool_capacity: int = 0, game_log: int = 0) -> None:
    if num_opponents == 0:
        raise ValueError("LeagueRollout needs at least one opponent (the no-opponent branch is select_actions' loop)")
    if len(opponent_ids) != num_opponents or len(set(opponent_ids)) != num_opponents:
        raise ValueError(f"opponent_ids must name each of the {num_opponents} opponents once, got {list(opponent_ids)}")
    if _lib.available():
        top = _lib.query("ka_league_layout", 4)
        if not 1 <= num_envs <= top:
            raise ValueError(f"num_envs must lie in [1, {top}], got {num_envs}")
    elif num_envs < 1:
        raise ValueError(f"num_envs must be positive, got {num_envs}")
    check_loop_args(max_ply, sync_every, graph, record, start_pool_capacity, game_log, one_truncation_slot=True)
    check_value_args(score_norm, value_adapter)


class LeagueRollout(DeviceRollout):
    """The learner's rollout against its league cohort, resident on the device (see module docstring).

    ``roll = LeagueRollout(learner, opponents, opponent_ids, num_envs=512, max_ply=500, ...)``;
    ``stats = roll.collect(buffer, steps)`` steps every env ``steps`` plies and leaves the learner's transitions in
    ``buffer`` (a device-resident ``KataGoRolloutBuffer``); ``roll.bootstrap_values()`` is the ``next_values`` of
    ``KataGoPPOAlgorithm.update``; ``roll.refresh()`` after the update brings the learner's new weights into the group;
    ``roll.set_opponents`` seats a new cohort.  The env is not reset between ``collect`` calls (the reference carries
    games over epochs); ``reset()`` is explicit.  ``seed`` fixes sampling and re-draws from the last ``reset()`` on.
    ``record=True`` (no graph) keeps every ply's inputs and outputs in ``self.record`` for tests.
    ``start_pool_capacity``, ``game_log``, ``move_history``, ``insight`` and ``insight_temperature`` are ``DevicePly``'s
    (``_device_ply.py``).  Here the log's launch is ``ka_gamelog_step_env`` and ``collect`` drains it onto
    ``LeagueRolloutStats.games``: a game names its players by id (``learner_id`` and ``opponent_ids``: the players who
    ended it, the ones its result is tallied for) and the learner's colour; it is ``carried`` where its side or its
    opponent changed in the middle of it (the epoch's side re-draw) and where it spans a ``set_opponents``.  The insight
    covers the learner's and the opponents' moves alike.
    ``opponent_sampling=`` (one ``SamplingControls`` for every opponent, or one per opponent; ``sampling.py``) has the
    opponents play through ``ka_policy_sample_ctl`` -- sharper, greedy or more diverse.  The learner's row of the controls
    table is always neutral, which is the play sampler bit for bit: its actions and the log-probs that reach the buffer stay
    draws from its own distribution, the PPO behaviour policy.  Without an option the ply is launch for launch what it is
    without it."""

    _LAYOUT = "ka_league_layout"

    def __init__(self, learner, opponents: Sequence, opponent_ids: Sequence[int], *, num_envs: int = 512, max_ply: int = 500,
                 value_adapter=None, score_norm: float = SCORE_NORMALIZATION, color_randomization: bool = False,
                 opponent_weights: Optional[Sequence[float]] = None, sync_every: int = 32, graph: bool = True,
                 seed: Optional[int] = None, record: bool = False, start_pool_capacity: int = 0, game_log: int = 0,
                 learner_id: int = -1, move_history: bool = False, insight: int = 0,
                 insight_temperature: float = 1.0, opponent_sampling=None) -> None:
        opponents, opponent_ids = list(opponents), [int(i) for i in opponent_ids]
        _check_args(len(opponents), opponent_ids, int(num_envs), int(max_ply), int(sync_every), bool(graph), bool(record),
                    float(score_norm), value_adapter, start_pool_capacity, game_log)
        self._ctl_host = league_controls(opponent_sampling, len(opponents))
        self._opponent_sampling = opponent_sampling
        self.learner_id = int(learner_id)
        self._cum_host = cum_thresholds(opponent_weights, len(opponents))
        self.learner, self.opponent_ids = learner, opponent_ids
        self.color_randomization = bool(color_randomization)
        q = lambda which: _lib.query("ka_league_layout", which)  # noqa: E731
        # the controls table of ka_policy_sample_ctl holds row 0, the learner, neutral
        self._build(self._make_group(learner, opponents), num_envs=num_envs, max_ply=max_ply, sync_every=sync_every,
                    graph=graph, seed=seed, record=record, value_adapter=value_adapter, score_norm=score_norm,
                    trunc_words=q(3), start_pool_capacity=int(start_pool_capacity), game_log=game_log, envs_per_slot=int(num_envs),
                    move_history=move_history, insight=insight, insight_temperature=insight_temperature,
                    controls=self._ctl_host)
        N, dev = self.num_envs, self.device
        with torch.cuda.device(dev):
            z = lambda *s, dtype=torch.int32: torch.zeros(*s, dtype=dtype, device=dev)  # noqa: E731
            self._side, self._opp, self._games = z(N, dtype=torch.uint8), z(N), z(N)
            self._p_obs, self._p_bits = z(N, *_OBS_SHAPE, dtype=torch.float32), z(N, MASK_WORDS)
            self._p_scal = z(q(2), N)
            self._side_host = torch.zeros(N, dtype=torch.uint8).pin_memory()
            self._every_env = z(1, 4)                             # a seat job naming the one slot of all envs
            self._ids: Optional[torch.Tensor] = None
        self._collects = 0
        self._seat_cohort()
        self._warm_up()

    # ------------------------------------------------------------------ cohort
    @staticmethod
    def _make_group(learner, opponents) -> SEResNetGroup:
        try:
            group = SEResNetGroup([learner, *opponents])
        except ValueError as e:
            raise ValueError(f"LeagueRollout needs the learner and every opponent as SEResNetModels of one shape on one "
                             f"GPU ({e}); use split_merge_step for this cohort") from e
        if group.device.type != "cuda" or group._tables is None:
            raise ValueError(f"LeagueRollout runs on a GPU group; these models are on {group.device}: use "
                             "split_merge_step for this cohort")
        return group

    def _seat_cohort(self) -> None:
        """Buffers whose size follows the number of opponents; the header of an existing state is kept."""
        K, dev = len(self.opponent_ids), self.device
        old = getattr(self, "_state", None)
        self._new_state(_lib.query("ka_league_state_words", K))
        with torch.cuda.device(dev):
            if old is not None:
                self._state[:_HDR].copy_(old[:_HDR])
            self._cum = torch.from_numpy(self._cum_host.view(np.int32).copy()).to(dev)
            if self.game_log is not None:                         # the ids the log names the players by: the same words
                ids = torch.tensor([self.learner_id, *self.opponent_ids], dtype=torch.int32)       # where K is unchanged
                if self._ids is None or self._ids.numel() != K + 1:
                    self._ids = ids.to(dev)
                else:
                    self._ids.copy_(ids)
        self._graphs = {}

    _KEEP = object()                                              # set_opponents(sampling=) not given

    def set_opponents(self, opponents: Sequence, opponent_ids: Sequence[int],
                      opponent_weights: Optional[Sequence[float]] = None, *, sampling=_KEEP) -> None:
        """A new cohort (epoch start): every env draws its opponent afresh; games in progress go on.  ``sampling=`` as
        the constructor's ``opponent_sampling``; without it a single ``SamplingControls`` stays in force, and a
        per-opponent list stays while the cohort keeps its size and is reset to neutral when the size changes."""
        opponents, opponent_ids = list(opponents), [int(i) for i in opponent_ids]
        _check_args(len(opponents), opponent_ids, self.num_envs, self.max_ply, self.sync_every, self.graph,
                    self.record_enabled, self.score_norm, self.value_adapter)
        cum = cum_thresholds(opponent_weights, len(opponents))
        if sampling is LeagueRollout._KEEP:
            sampling = self._opponent_sampling
            if not (sampling is None or isinstance(sampling, SamplingControls)) and len(sampling) != len(opponents):
                sampling = None
        self._ctl_host = league_controls(sampling, len(opponents))
        self._opponent_sampling = sampling
        same = len(opponents) + 1 == len(self.group) and all(a is b for a, b in zip(opponents, self.group.models[1:]))
        if not same:
            self.group = self._make_group(self.learner, opponents)
        else:
            self.group.refresh()
        self.opponent_ids, self._cum_host = opponent_ids, cum
        self.ply.seat(self.group, self._ctl_host)                 # a new workspace and table: the graphs are captured anew
        self._seat_cohort()
        with torch.cuda.device(self.device):
            if self.game_log is not None:                         # an unchanged index may name another model now: every game
                self.game_log.seat(self._every_env, 1)            # in progress is carried, whatever its env draws below
            games = self._games.cpu().numpy()
            self._opp.copy_(torch.from_numpy(draw_opponents(self._draw_seed, np.arange(self.num_envs), games, cum)))
            self._seat()

    # ------------------------------------------------------------------ state
    def reset(self) -> None:
        """Every env back to the start position, no pending transition, fresh seed, opponents and sides drawn anew."""
        N, dev = self.num_envs, self.device
        seed = self._fresh_seed()
        self._draw_seed = int(seed)
        with torch.cuda.device(dev):
            hdr = torch.zeros(self._state.shape, dtype=torch.int32)
            hdr[_SEED:_SEED + 2].view(torch.int64)[0] = seed
            hdr[_DRAW_SEED:_DRAW_SEED + 2].view(torch.int64)[0] = seed
            self._state.copy_(hdr)
            self._desc.zero_()
            self._p_scal.zero_()
            self._games.zero_()
            self._stall.zero_()
            envs = np.arange(N)
            self._opp.copy_(torch.from_numpy(draw_opponents(seed, envs, np.zeros(N, np.int64), self._cum_host)))
            side = draw_sides(seed, envs, np.zeros(N, np.int64)) if self.color_randomization else np.zeros(N, np.uint8)
            self._side.copy_(torch.from_numpy(side))
            self.ply.reset()
            self._seat()
        self._collects = 0
        self.record = []

    def _seat(self) -> None:
        """model_of of the ply to come from the current players, sides and opponents."""
        players = self.env._players[self.env._cur]
        self._model_of.copy_(torch.where(players == self._side, torch.zeros_like(self._opp), self._opp + 1))

    @property
    def last_values(self) -> torch.Tensor:
        """The learner's value of the last ply where it moved, 0 elsewhere (the reference's ``latest_values``)."""
        return self._values

    # ------------------------------------------------------------------ one ply
    def _ply(self) -> None:
        """forward -> sample -> step -> league bookkeeping on the current stream; no host synchronisation."""
        ply, N, K = self.ply, self.num_envs, len(self.opponent_ids)
        sp = self._state.data_ptr()
        cur, pre, value, score, st = ply.move(self._model_of, K + 1, sp, sp + 4 * self._SAMP)
        r = ply.step()
        # before ka_league_step re-draws side and opp of finished envs
        ply.log(r, pre, side=self._side, opp=self._opp, ids=self._ids, opponents=K, ply_counter=sp + 4 * _PLY)
        _lib.call("ka_league_step", self._state, N, K, 0, cur.observations, cur.legal_mask_bits, self._actions, self._logp,
                  value, score if self.alpha != 0.0 else None, self.alpha, self._nlegal, pre, r.rewards,
                  r.terminated, r.truncated, r.current_players, r.step_metadata.material_balance, self.score_norm,
                  r.terminal_observations, self.env._err.data_ptr() + 8, self._side, self._opp, self._games, self._cum,
                  int(self.color_randomization), self._model_of, self._stall, self._values, self._p_obs, self._p_bits,
                  self._p_scal, self._t_obs, self._t_list, self._desc, self._plan, _OBS_ELEMS, MASK_WORDS, st)

    def _ply_recorded(self) -> None:
        env = self.env
        cur, prev = env.current(), env._cur
        rec = {"seed": int(self._state[:2].view(torch.int64).item()), "obs": cur.observations.cpu(),
               "mask_bits": cur.legal_mask_bits.cpu(), "model_of": self._model_of.cpu().numpy(),
               "pre_players": env._players[prev].cpu().numpy(), "side": self._side.cpu().numpy(),
               "opp": self._opp.cpu().numpy(),
               "game_plies": env._state[:, GAME_PLY_BYTE:GAME_PLY_BYTE + 4].cpu().contiguous().view(torch.int32).reshape(-1).numpy()}
        self._ply()
        c = env._cur
        trunc = (env._truncated[c] & ~env._terminated[c]).nonzero(as_tuple=True)[0]
        rec.update(actions=self._actions.cpu().numpy(), log_probs=self._logp.cpu().numpy(), values=self._values.cpu().numpy(),
                   n_legal=self._nlegal.cpu().numpy(), rewards=env._rewards[c].cpu().numpy(),
                   terminated=env._terminated[c].cpu().numpy(), truncated=env._truncated[c].cpu().numpy(),
                   current_players=env._players[c].cpu().numpy(), material=env._material[c].cpu().numpy(),
                   terminal_envs=trunc.cpu().numpy(), terminal_obs=env._terminal_obs[trunc].cpu(),
                   reason=env._reason[c].cpu().numpy(), state=env._state[:, :POOL_ROW_BYTES].cpu().numpy())
        self.record.append(rec)

    # ------------------------------------------------------------------ host side
    def _zero_legal(self, st: np.ndarray) -> None:
        if st[_STALL]:
            stall = self._stall.cpu().numpy()
            for bit, who in ((1, "Learner"), (2, "Opponent")):
                if st[_STALL] & bit:
                    raise RuntimeError(_ZERO_LEGAL.format(who=who, envs=np.flatnonzero(stall & bit).tolist()))

    def _protocol_guards(self, st: np.ndarray) -> None:
        if st[_CONFLICT]:
            PendingTransitions._conflict()

    def _overrides(self, cols: dict, n: int) -> None:
        """The deferred truncation bootstrap (:1250-1283): one learner forward over the n parked terminal observations,
        sign-corrected to the learner's frame, scattered into the rows' next_value_override."""
        tl = self._t_list[:n]
        v = self._learner_values(self._t_obs[:n], n, None)
        who = tl[:, 2]
        v = torch.where((who & 1) != (who >> 1), -v, v)          # sign_correct_bootstrap(term_v, 1 - pre_players, side)
        cols["next_value_override"].index_copy_(0, tl[:, 1].long(), v)
        self._state[_TRUNC:_TRUNC + 1].zero_()

    def collect(self, buffer: KataGoRolloutBuffer, steps: int) -> LeagueRolloutStats:
        """Step every env ``steps`` plies; the learner's transitions land in ``buffer`` in the reference's order."""
        self._check_buffer(buffer, steps)
        return self._run_collect(buffer, steps, LeagueRolloutStats())

    def _collect(self, buffer, steps, stats) -> None:
        N = self.num_envs
        self.record = []
        self._state[_ROWS:_SAMP + 2].zero_()
        self._state[_TRUNC:].zero_()
        self._stall.zero_()
        if self.color_randomization:                              # katago_loop.py:1134-1137: all sides anew every epoch
            self._side_host.copy_(torch.from_numpy(draw_sides(self._draw_seed, np.arange(N), np.full(N, self._collects),
                                                              SALT_EPOCH_SIDE)))
            self._side.copy_(self._side_host, non_blocking=True)
            self._seat()
        self._collects += 1
        base, rows, adds, done = buffer._write_offset, 0, 0, 0
        dropped_before = self.game_log.dropped if self.game_log is not None else 0

        def sync(cols):
            nonlocal rows, adds
            st = self._read_state(stats)
            buffer.commit(int(st[_ROWS]) - rows, int(st[_BLOCKS]) - adds)
            rows, adds = int(st[_ROWS]), int(st[_BLOCKS])
            self._after_commit(st, cols, stats, dropped_before)
            return st

        while done < steps:
            plies = min(self.sync_every, steps - done)
            cols = self._describe(buffer, base, plies * N)
            self._chunk(plies)
            sync(cols)
            done += plies
        cols = self._describe(buffer, base, N)                   # :1537-1563: what is still pending leaves with done = 0
        _lib.call("ka_league_step", self._state, N, len(self.opponent_ids), 1, *([None] * 6), 0.0, *([None] * 7), 1.0,
                  *([None] * 6), 0, None, None, None, self._p_obs, self._p_bits, self._p_scal, None, None, self._desc,
                  self._plan, _OBS_ELEMS, MASK_WORDS, _lib.stream_ptr(self.device))
        before = rows
        st = sync(cols)
        stats.plies, stats.flushed, stats.adds = steps, rows - before, int(st[_BLOCKS])
        self._tallies(st, stats)
        stats.opponent_results = {oid: [int(v) for v in st[_HDR + 3 * k:_HDR + 3 * k + 3]]
                                  for k, oid in enumerate(self.opponent_ids)}

    def live_games(self, envs: Optional[Sequence[int]] = None) -> List[RecordedGame]:
        """The games in progress (every env, or ``envs``) between two ``collect`` calls: ``RecordedGame`` with
        ``finished=False``, named by the players seated now."""
        return self.ply.live_games("a rollout", envs, side=self._side, opp=self._opp, ids=self._ids,
                                   opponents=len(self.opponent_ids), ply_counter=self._state.data_ptr() + 4 * _PLY)

    def spectator_data(self, envs: Optional[Sequence[int]] = None) -> List[dict]:
        """``DevicePly.spectator_data`` between two ``collect`` calls."""
        return self.ply.spectator_data(envs)

    def bootstrap_values(self) -> torch.Tensor:
        """V(observation now) by the learner, in the learner's frame (katago_loop.py:1565-1580): ``update``'s next_values."""
        with torch.cuda.device(self.device), torch.no_grad():
            env = self.env
            v = self._learner_values(env.current().observations, self.num_envs, self._ws)
            return torch.where(env._players[env._cur] != self._side, -v, v)


# ---------------------------------------------------------------------------------------------- host restatement
def _league_host(records: Sequence[dict], *, num_envs: int, obs_shape: tuple, action_space: int, opponent_ids: Sequence[int],
                 seed: int, cum: np.ndarray, color_randomization: bool, score_norm: float, side: np.ndarray,
                 opp: np.ndarray, games: Optional[np.ndarray] = None, trace: Optional[list] = None):
    """The reference's rollout protocol (katago_loop.py:1219-1437, :1537-1563) over per-ply records, on the CPU, from
    this package's host pieces.  A record holds one ply as arrays over all envs: ``obs``, ``mask_bits`` (packed int32
    rows) or ``legal_masks`` (bool), ``pre_players``, ``actions``, ``log_probs``, ``values``, ``rewards``, ``terminated``,
    ``truncated``, ``current_players``, ``material`` and, for plies with truncations, ``term_values`` (the learner's value
    of every env's terminal observation, before the sign correction; NaN where there is none).  ``side`` / ``opp`` /
    ``games``: the per-env learner side, opponent index and finished-game count before the first record.
    Returns ``(columns, stats)``: the host buffer's ``flatten()`` plus ``size``, and the tallies as a dict.  ``trace`` (a
    list) receives per ply the state after it: side, opp, games, model_of and the pending slots' valid flags."""
    t = lambda x, dt=None: torch.as_tensor(np.asarray(x), dtype=dt)  # noqa: E731
    dev = torch.device("cpu")
    K = len(opponent_ids)
    side, opp = np.array(side, dtype=np.uint8), np.array(opp, dtype=np.int32)
    games = np.zeros(num_envs, np.int64) if games is None else np.array(games, dtype=np.int64)
    pending = PendingTransitions(num_envs, tuple(obs_shape), action_space, dev)
    buffer = KataGoRolloutBuffer(num_envs, tuple(obs_shape), action_space)
    tally = dict(wins=0, losses=0, draws=0, black_wins=0, white_wins=0, terminated=0, truncated=0, truncation_overrides=0)
    results = {oid: [0, 0, 0] for oid in opponent_ids}
    envs = np.arange(num_envs)

    def add(fin, cats, override):
        buffer.add(fin["obs"], fin["actions"], fin["log_probs"], fin["values"], fin["rewards"], fin["dones"],
                   fin["terminated"], fin["legal_masks"], cats, fin["score_targets"], env_ids=fin["env_ids"],
                   next_value_override=override)

    for rec in records:
        pre, cur = np.asarray(rec["pre_players"]).astype(np.uint8), np.asarray(rec["current_players"]).astype(np.uint8)
        learner_moved, learner_next = t(pre == side), t(cur == side)
        rewards = t(rec["rewards"], torch.float32)
        terminated, truncated = t(rec["terminated"]).bool(), t(rec["truncated"]).bool()
        dones = terminated | truncated
        tally["terminated"] += int(terminated.sum())
        tally["truncated"] += int((truncated & ~terminated).sum())
        learner_rewards = to_learner_perspective(rewards, pre, side)
        if terminated.any():                                     # :1226-1248
            tr = learner_rewards[terminated]
            tally["wins"] += int((tr > 0).sum()); tally["losses"] += int((tr < 0).sum()); tally["draws"] += int((tr == 0).sum())
            raw, who = rewards[terminated], t(pre)[terminated]
            tally["black_wins"] += int((((raw > 0) & (who == 0)) | ((raw < 0) & (who == 1))).sum())
            tally["white_wins"] += int((((raw > 0) & (who == 1)) | ((raw < 0) & (who == 0))).sum())
        truncated_only = truncated & ~terminated
        override_full = None
        if bool(truncated_only.any()):                           # :1258-1283
            term_v = sign_correct_bootstrap(t(rec["term_values"], torch.float32), 1 - pre, side)
            override_full = torch.full_like(term_v, float("nan"))
            override_full[truncated_only] = term_v[truncated_only]
        pending.accumulate_reward(learner_rewards)               # :1290-1316
        fin = pending.finalize(pending.valid & (dones | learner_next), dones, terminated)
        if fin is not None:
            ov = override_full[fin["env_ids"]] if override_full is not None else None
            tally["truncation_overrides"] += 0 if ov is None else int((~torch.isnan(ov)).sum())
            add(fin, _compute_value_cats(fin["rewards"], fin["terminated"].bool(), dev), ov)
        if learner_moved.any():                                  # :1319-1365
            masks = t(rec["mask_bits"], torch.int32) if "mask_bits" in rec else t(rec["legal_masks"]).bool()
            zero = torch.zeros(num_envs)
            pending.create(learner_moved, t(rec["obs"], torch.float32), t(rec["actions"], torch.long),
                           torch.where(learner_moved, t(rec["log_probs"], torch.float32), zero),
                           torch.where(learner_moved, t(rec["values"], torch.float32), zero), masks, learner_rewards,
                           t(rec["material"]).to(torch.float32) / score_norm)
            imm = learner_moved & dones
            if imm.any():
                fin = pending.finalize(imm, dones, terminated)
                if fin is not None:
                    ov = override_full[fin["env_ids"]] if override_full is not None else None
                    tally["truncation_overrides"] += 0 if ov is None else int((~torch.isnan(ov)).sum())
                    add(fin, _compute_value_cats(fin["rewards"], fin["terminated"].bool(), dev), ov)
        done_np = dones.numpy()
        for e in np.flatnonzero(done_np):                        # :1384-1407: by the opponent that played the game
            if terminated[e]:
                lr = float(learner_rewards[e])
                results[opponent_ids[opp[e]]][0 if lr > 0 else (1 if lr < 0 else 2)] += 1
        if done_np.any():                                        # :1409-1437: the next game's opponent and side
            games[done_np] += 1
            opp[done_np] = draw_opponents(seed, envs[done_np], games[done_np], cum)
            if color_randomization:
                side[done_np] = draw_sides(seed, envs[done_np], games[done_np])
        if trace is not None:
            trace.append(dict(side=side.copy(), opp=opp.copy(), games=games.copy(),
                              model_of=np.where(cur == side, 0, opp + 1).astype(np.int32),
                              valid=pending.valid.numpy().copy(), rewards=pending.rewards.numpy().copy(),
                              obs=pending.obs.numpy().copy(), mask_bits=pending.legal_mask_bits.numpy().copy(),
                              actions=pending.actions.numpy().copy(), log_probs=pending.log_probs.numpy().copy(),
                              values=pending.values.numpy().copy(), score_targets=pending.score_targets.numpy().copy()))
    if bool(pending.valid.any()):                                # :1537-1563
        zero = torch.zeros(num_envs)
        fin = pending.finalize(pending.valid.clone(), zero, zero)
        if fin is not None:
            add(fin, torch.full((fin["env_ids"].numel(),), -1, dtype=torch.long), None)
    cols = dict(buffer.flatten()) if buffer.size else {}
    cols["size"] = buffer.size
    stats = dict(tally, plies=len(records), rows=buffer._write_offset, adds=buffer.size,
                 opponent_results={k: list(v) for k, v in results.items()})
    return cols, stats
