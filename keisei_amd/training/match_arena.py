"""MatchArena: league matches played on the device, many pairings at once (the reference's
``ConcurrentMatchPool.run_round``, concurrent_matches.py:196-545).

The arena owns one device ``VecEnv`` split into ``num_envs // envs_per_match`` contiguous slots (env b belongs to slot
``b // envs_per_match``, as ``partition_range``).  Each slot plays one pairing ``(a, b)`` of models of an
``SEResNetGroup``: model a moves for player 0, model b for player 1.  One ply is four steps on one stream, with no host
synchronisation:

    grouped stem / tower / heads on model_of   (csrc/tower.hip, SEResNetGroup's tables)
    ka_policy_sample_play                       (csrc/loss.hip: seed read from the device; unseated rows take their
                                                 first legal action, as the reference does for idle partitions;
                                                 with sampling= its place is taken by ka_policy_sample_ctl,
                                                 csrc/sampling.hip: temperature, top-k cut and opening plies per model)
    tree search                                 (only with search=, in the lookahead's place: per expansion a fork
                                                 (ka_lookahead_fork, then ka_search_expand), ka_shogi_env_step and the
                                                 grouped forward over its slice of the node pool, ka_search_advance --
                                                 csrc/lookahead.hip, tree_search.py)
    visit-count search                          (only with mcts=, in the same place: the same stages per simulation with
                                                 ka_mcts_advance as the tree policy -- csrc/mcts.hip, mcts_search.py)
    lookahead                                   (only with lookahead=: ka_lookahead_fork, ka_shogi_env_step over the child
                                                 rows, the grouped forward over the child observations,
                                                 ka_lookahead_choose -- or, with a reply_width, three more stages over the
                                                 grandchild rows and ka_lookahead_choose_replies -- csrc/lookahead.hip,
                                                 lookahead.py: the models with a
                                                 width play the best of their top moves by their own value head)
    mate in one                                 (only with mate=: ka_mate_fork, ka_shogi_env_step over the child rows,
                                                 ka_mate_choose -- csrc/mate.hip, mate_search.py: a model with
                                                 max_checks > 0 plays a mate in one when the rules say there is one,
                                                 whatever the sampler, the lookahead or the search chose)
    mate in three                               (only with mate= and an evasion_rows > 0: ka_mate3_fork, ka_shogi_env_step
                                                 over the grandchild rows, ka_mate3_gate, the three mate-in-one stages
                                                 over the grandchild rows, ka_mate3_choose -- csrc/mate3.hip: the lowest
                                                 check after which every reply runs into a mate in one)
    ka_shogi_env_step                           (csrc/shogi_env.hip)
    ka_arena_features_step                      (csrc/arena.hip, only with features=True: the reference's per-slot
                                                 GameFeatureTracker, one record per finished game)
    ka_search_sample_step                       (csrc/search_samples.hip, only with search_samples > 0: the searched
                                                 positions with their visit counts, labelled when their game ends)
    ka_gamelog_step                             (csrc/gamelog.hip, only with game_log > 0: the finished games, move
                                                 by move, one record per game the referee tallies)
    ka_arena_referee                            (csrc/arena.hip: tally by the last-mover rule, close slots, seat the
                                                 next ply, advance the seed)

The host looks in every ``sync_every`` plies with one read of the arena's state array.  It turns finished slots into
results and seats the next pairings, in priority order, in the freed slots.  The order is the reference's: finished
slots are taken in reverse order of their place in the active list, and a refilled slot goes to the end of that list.

Deviation from the reference: a slot that finishes between two sync points sits idle (its envs take their first legal
action) until the next sync, where the reference swaps the next pairing in at once.  ``sync_every=2`` is the closest
schedule a captured graph allows (``VecEnv`` alternates two result buffers, so a graph must hold an even number of
plies); ``graph=False, sync_every=1`` is the reference's schedule exactly.  As in the reference there is one
``reset()`` per round and no per-slot reset: a pairing seated in a freed slot continues the games in progress there.

The front of the ply (forward, sampler, lookahead, insight, env step, game log) is ``_device_ply.DevicePly``, shared with
``LeagueRollout`` and ``SelfPlayRollout``; the arena adds its collection and feature launches, the referee, its own
single-graph capture and the round.
"""
from __future__ import annotations

import time
from dataclasses import dataclass
from typing import Callable, Dict, List, Mapping, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from keisei_amd import _lib
from keisei_amd.shogi_gym import MASK_WORDS

from ._device_ply import _OBS_ELEMS, DevicePly, check_loop_args
from .dynamic_trainer import MatchRollout
from .game_feature_tracker import GameFeatureTracker
from .game_log import RecordedGame
from .lookahead import LookaheadStage, LookaheadStats
from .mate_search import Mate3Stats, MateStage, MateStats
from .mcts_explore import arena_mcts_explore
from .mcts_search import MctsStage, MctsStats
from .model_group import SEResNetGroup
from .sampling import GAME_PLY_BYTE, arena_controls, controls_table
from .search_samples import arena_search_samples
from .tree_search import SearchStage, SearchStats

_HDR, _SLOT = 8, 8                      # int32 words of the state header and of one slot (csrc/arena.hip)
_PLY, _MAX_PLY, _SAMP, _REFUSAL = 2, 3, 4, 6    # header words: plies of the round, the ply ceiling's max_ply, the
                                        # sampler's two flags, the env's refusal latch (int64)
_CUR = 4                                # int32 words of one slot's collection cursors: rows, rows of this ply, dropped, -
DONE, PARTIAL = 2, 4                   # slot status bits (csrc/arena.hip; 1 = seated, 8 = stalled)


@dataclass
class MatchResult:
    """One pairing's result (the reference's MatchResult with model indices in place of opponent entries)."""
    a: int
    b: int
    a_wins: int
    b_wins: int
    draws: int
    plies: int
    partial: bool
    rollout: Optional[MatchRollout] = None      # collected rows (flat, packed masks, on the arena's device)
    feature_tracker: Optional[GameFeatureTracker] = None     # the pairing's game features (arenas with features=True)
    # the pairing's finished games, move by move, in (ply, env) order (arenas with game_log > 0, else None).  The name
    # `games` is taken by the count below.
    recorded_games: Optional[List[RecordedGame]] = None

    @property
    def games(self) -> int:
        return self.a_wins + self.b_wins + self.draws


@dataclass
class RoundStats:
    round_duration_s: float = 0.0
    pairings_requested: int = 0
    pairings_completed: int = 0
    total_games: int = 0
    total_plies: int = 0                # sum of the pairings' plies
    round_plies: int = 0                # plies the arena stepped (a multiple of sync_every)
    host_syncs: int = 0                 # reads of the state array
    active_slots: int = 0
    rollout_rows: int = 0               # rows handed out in rollouts
    rollouts_dropped: int = 0           # pairings whose rollout was withheld because the store lost rows of it
    feature_rows: int = 0               # rows handed out in feature trackers (two per finished game)
    features_dropped: int = 0           # finished games whose record did not fit the feature store
    games_dropped: int = 0              # finished games that did not fit the game log between two sync points
    lookahead: Optional[LookaheadStats] = None      # the round's lookahead counters (arenas built with lookahead=)
    search: Optional[SearchStats] = None            # the round's tree-search counters (arenas built with search=)
    mcts: Optional[MctsStats] = None                # the round's visit-count search counters (arenas built with mcts=)
    mate: Optional[MateStats] = None                # the round's mate-in-one counters (arenas built with mate=)
    mate3: Optional[Mate3Stats] = None              # the round's mate-in-three counters (mate= with evasion_rows > 0)


def _side_bits(trainable, pairings: Sequence[Tuple[int, int]]) -> List[int]:
    """Per pairing: bit 0 = collect side A's rows, bit 1 = side B's.  ``trainable``: None, a callable ``(a, b) -> int``
    (the reference's trainable_fn, concurrent_matches.py:610-612, with the side in the answer) or a mapping from pairing
    index to the bits."""
    if trainable is None:
        return [0] * len(pairings)
    if callable(trainable):
        bits = [int(trainable(a, b)) for a, b in pairings]
    else:
        bits = [int(trainable.get(i, 0)) for i in range(len(pairings))]
        extra = [k for k in trainable if not (isinstance(k, int) and 0 <= k < len(pairings))]
        if extra:
            raise ValueError(f"trainable names pairing indices {extra} outside [0, {len(pairings)})")
    for i, b in enumerate(bits):
        if not 0 <= b <= 3:
            raise ValueError(f"trainable gives {b} for pairing {i}: side bits are 0..3 (1 = side A, 2 = side B)")
    return bits


def _check_round(pairings: Sequence[Tuple[int, int]], games_per_match: int, num_models: int) -> List[Tuple[int, int]]:
    if games_per_match <= 0:
        raise ValueError(f"games_per_match must be positive, got {games_per_match}")
    out = []
    for i, p in enumerate(pairings):
        a, b = (int(x) for x in p)
        if not (0 <= a < num_models and 0 <= b < num_models):
            raise ValueError(f"pairing {i} = ({a}, {b}): model indices must lie in [0, {num_models})")
        out.append((a, b))
    return out


def _ceiling(max_ply: int, target: int, envs: int) -> int:
    return max_ply * (-(-target // max(1, envs)) + 1)          # concurrent_matches.py:473-480


def _referee_host(records: Sequence[dict], pairings: Sequence[Tuple[int, int]], *, num_slots: int, envs_per_slot: int,
                  games_per_match: int, max_ply: int, sync_every: int = 1, trace: Optional[list] = None):
    """The reference's per-ply bookkeeping (concurrent_matches.py:254-506) restated in plain Python over per-ply records,
    with the swap-in moved to the sync points (every ``sync_every`` plies) as the arena does it.

    Each record holds the env facts of one ply as numpy arrays over all envs: ``pre_players`` (the player to move before
    the step), ``n_legal`` (legal actions before the step; optional), ``rewards``, ``terminated``, ``truncated``.
    Returns ``(results, seating)``: results[i] = (a_wins, b_wins, draws, plies, partial) of pairing i, or None if it never
    finished within the records; seating[t] = the model index each env plays with at ply t (-1 = unseated).  ``trace``
    (a list) receives per ply the ``{slot index: pairing index}`` of the slots that stepped."""
    P = len(pairings)
    slots = [dict(index=i, start=i * envs_per_slot, end=(i + 1) * envs_per_slot, pairing=None, a_wins=0, b_wins=0,
                  draws=0, target=0, plies=0, finished=False, partial=False) for i in range(min(num_slots, P))]
    results: List[Optional[tuple]] = [None] * P
    nxt = 0

    def assign(slot):
        nonlocal nxt
        slot.update(pairing=nxt, a_wins=0, b_wins=0, draws=0, target=games_per_match, plies=0, finished=False, partial=False)
        nxt += 1

    active = []
    for slot in slots:
        assign(slot)
        active.append(slot)
    seating = []
    for t, rec in enumerate(records):
        n = len(rec["rewards"])
        seat = np.full(n, -1, dtype=np.int64)
        live = [s for s in active if not s["finished"]]
        stepped = set()
        for s in live:
            s["plies"] += 1
        for s in live:
            lo, hi = s["start"], s["end"]
            nl = rec.get("n_legal")
            if nl is not None and (np.asarray(nl[lo:hi]) == 0).any():       # zero-legal guard: target = games so far
                s["target"] = s["a_wins"] + s["b_wins"] + s["draws"]
                continue
            stepped.add(s["index"])
            a, b = pairings[s["pairing"]]
            pp = np.asarray(rec["pre_players"][lo:hi])
            seat[lo:hi] = np.where(pp == 0, a, b)
        seating.append(seat)
        if trace is not None:
            trace.append({s["index"]: s["pairing"] for s in live if s["index"] in stepped})
        for s in live:
            if s["index"] in stepped:
                lo, hi = s["start"], s["end"]
                done = np.asarray(rec["terminated"][lo:hi]) | np.asarray(rec["truncated"][lo:hi])
                for k in np.flatnonzero(done):
                    r = float(rec["rewards"][lo + k])
                    a_moved = int(rec["pre_players"][lo + k]) == 0
                    if r > 0:
                        s["a_wins" if a_moved else "b_wins"] += 1
                    elif r < 0:
                        s["b_wins" if a_moved else "a_wins"] += 1
                    else:
                        s["draws"] += 1
            if s["a_wins"] + s["b_wins"] + s["draws"] >= s["target"]:
                s["finished"] = True
            elif s["plies"] >= _ceiling(max_ply, s["target"], s["end"] - s["start"]):
                s["finished"] = s["partial"] = True
        if (t + 1) % sync_every == 0:
            for i in sorted((i for i, s in enumerate(active) if s["finished"]), reverse=True):
                s = active.pop(i)
                results[s["pairing"]] = (s["a_wins"], s["b_wins"], s["draws"], s["plies"], s["partial"])
                if nxt < P:
                    assign(s)
                    active.append(s)
    return results, seating


def _rollout_rows_host(records: Sequence[dict], pairings: Sequence[Tuple[int, int]], bits: Sequence[int], *,
                       num_slots: int, envs_per_slot: int, games_per_match: int, max_ply: int, sync_every: int = 1):
    """The record rule of ``ka_arena_record_pre`` restated over ``_referee_host``'s bookkeeping: per pairing, the
    ``(ply, env)`` pairs of its rollout rows, in order.  A slot that steps at ply t (seated, not finished, no env without
    a legal action) gives one row per env whose pre-step player p has bit p of the pairing's side bits set."""
    trace: List[dict] = []
    _referee_host(records, pairings, num_slots=num_slots, envs_per_slot=envs_per_slot, games_per_match=games_per_match,
                  max_ply=max_ply, sync_every=sync_every, trace=trace)
    rows: List[List[Tuple[int, int]]] = [[] for _ in pairings]
    for t, (rec, stepped) in enumerate(zip(records, trace)):
        for slot, p in sorted(stepped.items()):
            for e in range(slot * envs_per_slot, (slot + 1) * envs_per_slot):
                if (bits[p] >> (int(rec["pre_players"][e]) & 1)) & 1:
                    rows[p].append((t, e))
    return rows


def _entry_id(entry_ids, model: int) -> int:
    return model if entry_ids is None else entry_ids[model]


def _features_host(records: Sequence[dict], pairings: Sequence[Tuple[int, int]], *, num_slots: int, envs_per_slot: int,
                   games_per_match: int, max_ply: int, sync_every: int = 1, entry_ids=None,
                   epoch: int = 0) -> List[GameFeatureTracker]:
    """The reference's feature tracking (concurrent_matches.py:125-130, :441-452) over ``_referee_host``'s bookkeeping:
    one host ``GameFeatureTracker`` per pairing, made when the pairing is seated, and ``record_step`` on the envs of
    every slot that stepped.  The records carry ``actions``, ``captured_piece``, ``termination_reason`` and ``ply_count``
    beside what ``_referee_host`` reads.  Returns the trackers in pairing order."""
    trace: List[dict] = []
    _referee_host(records, pairings, num_slots=num_slots, envs_per_slot=envs_per_slot, games_per_match=games_per_match,
                  max_ply=max_ply, sync_every=sync_every, trace=trace)
    trackers = [GameFeatureTracker(envs_per_slot, _entry_id(entry_ids, a), _entry_id(entry_ids, b), epoch)
                for a, b in pairings]                           # a pairing is seated once: its tracker is new then
    for rec, stepped in zip(records, trace):
        for slot, p in sorted(stepped.items()):
            lo, hi = slot * envs_per_slot, (slot + 1) * envs_per_slot
            trackers[p].record_step(*(np.asarray(rec[k][lo:hi]) for k in (
                "actions", "captured_piece", "termination_reason", "ply_count", "pre_players", "terminated", "truncated",
                "rewards")))
    return trackers


class MatchArena:
    """Concurrent league matches over one device ``VecEnv`` (see module docstring).

    ``arena = MatchArena(group, num_envs, envs_per_match, max_ply, sync_every=32, graph=True, seed=None)``;
    ``results, stats = arena.run_round(pairings, games_per_match)``.  ``seed`` fixes the round's sampling (each round
    draws a fresh one from torch's host generator when it is None).  ``graph=True`` captures ``sync_every`` plies once
    as a CUDA graph and replays it; ``sync_every`` must then be even.  ``record=True`` (no graph) keeps every ply's
    inputs and outputs in ``self.record`` for tests.  ``collect=True`` adds rollout collection to the ply (two launches,
    ``ka_arena_record_pre`` / ``ka_arena_record_post``, into a store allocated here) for ``run_round(trainable=)``.
    ``features=True`` adds the reference's per-slot ``GameFeatureTracker`` to the ply (one launch,
    ``ka_arena_features_step``): every result then carries a ``feature_tracker``.  Without it the ply is launch for
    launch what it was.  ``start_pool_capacity``, ``game_log``, ``move_history``, ``insight`` and ``insight_temperature``
    are ``DevicePly``'s (``_device_ply.py``).  Here ``start_pool_capacity`` is not for ``features=True``; the log's launch
    is ``ka_gamelog_step`` and every result carries its pairing's finished games, move by move, in ``recorded_games`` --
    one per game the referee tallied, as long as ``RoundStats.games_dropped`` is 0.  A game is ``carried`` when the pairing
    inherited it from the slot's previous pairing or the slot sat idle during it (there is no per-slot reset).
    ``collect``, ``features`` and ``game_log`` are independent.  The ``insight`` of ``spectator_data()`` is None for the
    envs of an idle slot.
    The options that change how a move is chosen are per model, each described in its module.  None leaves the ply launch
    for launch what it was; every row off allocates nothing and launches nothing; none goes with ``collect=True``; each
    ``set_*`` rewrites the option's table on the device between two rounds without a new capture, up to the sizes built.
    ``sampling=`` (``sampling.py``, ``set_sampling``): temperature, top-k cut and opening schedule, ``ka_policy_sample_ctl``.
    ``lookahead=`` (``lookahead.py``, ``set_lookahead``): the best of the top moves by the model's own value head, with a
    ``reply_width`` over two plies.
    ``search=`` (``tree_search.py``, ``set_search``): a best-first minimax search where the lookahead stands.
    ``mcts=`` (``mcts_search.py``, ``set_mcts``): a visit-count (PUCT) search in the same place; ``arena.mcts`` is its engine.
    ``mcts_explore=`` (``mcts_explore.py``, ``set_mcts_explore``; only with ``mcts=``): root noise and visit-proportional play.
    ``search_samples=rows_per_env`` (``search_samples.py``; only with ``mcts=``): the searched positions as training rows,
    ``arena.search_samples.drain()`` between two rounds.
    ``mate=`` (``mate_search.py``, ``set_mate``): a rules-only mate in one, and in three, that overrides whatever was chosen.
    At most one of ``lookahead=``, ``search=`` and ``mcts=``.  The searches are the ``PlyStage`` objects of
    ``arena.ply.stages`` (``_forked_rows.py``), by name, in launch order; their counters are the ``RoundStats`` fields."""

    def __init__(self, group: SEResNetGroup, num_envs: int = 512, envs_per_match: int = 64, max_ply: int = 512, *,
                 sync_every: int = 32, graph: bool = True, seed: Optional[int] = None, record: bool = False,
                 collect: bool = False, features: bool = False, start_pool_capacity: int = 0,
                 game_log: int = 0, move_history: bool = False, insight: int = 0,
                 insight_temperature: float = 1.0, sampling=None, lookahead=None, search=None, mate=None,
                 mcts=None, search_samples: int = 0, mcts_explore=None) -> None:
        if len(group) == 0:
            raise ValueError("MatchArena needs a group with at least one model")
        if num_envs <= 0 or envs_per_match <= 0 or num_envs % envs_per_match != 0:
            raise ValueError(f"num_envs ({num_envs}) must be a positive multiple of envs_per_match ({envs_per_match})")
        check_loop_args(max_ply, sync_every, graph, record, start_pool_capacity, game_log)
        K, collect = len(group), bool(collect)
        search_samples = arena_search_samples(search_samples, mcts, K)
        explore = arena_mcts_explore(mcts_explore, mcts, K)
        if features and start_pool_capacity > 0:
            raise ValueError("features=True cannot be combined with start_pool_capacity > 0: the opening and rook-square "
                             "style features are defined from the standard start position")
        if group.device.type != "cuda" or group._tables is None:
            raise ValueError(f"MatchArena runs on a GPU group; this group is on {group.device} (VecEnv has no CPU path)")
        table = arena_controls(sampling, K, collect)
        # the searches of the ply, in launch order (None: not given); DevicePly refuses two in the lookahead's place
        stages = (LookaheadStage.parse(lookahead, K, collect), SearchStage.parse(search, K, collect),
                  MctsStage.parse(mcts, K, collect, explore), MateStage.parse(mate, K, collect))
        self.group = group
        self.device = group.device
        self.num_envs, self.envs_per_match, self.max_ply = int(num_envs), int(envs_per_match), int(max_ply)
        self.num_slots = self.num_envs // self.envs_per_match
        self.sync_every, self.graph, self.seed = int(sync_every), bool(graph), seed
        self.record_enabled = bool(record)
        self.record: List[dict] = []
        N, dev = self.num_envs, self.device
        # the controls table of ka_policy_sample_ctl and the stages' tables are allocated once: the set_* methods write
        # into them, the ply reads them
        self.ply = ply = DevicePly(group, N, self.max_ply, start_pool_capacity=int(start_pool_capacity), game_log=game_log,
                                   envs_per_slot=self.envs_per_match, move_history=move_history, insight=insight,
                                   insight_temperature=insight_temperature, controls=table, stages=stages,
                                   search_samples=int(search_samples))
        self.env, self.game_log, self.insight = ply.env, ply.game_log, ply.insight
        self._actions, self._logp, self._nlegal = ply.actions, ply.log_probs, ply.n_legal
        self._ctl, self.mcts, self.search_samples = ply.ctl, ply.mcts, ply.search_samples
        with torch.cuda.device(dev):
            self._state = torch.zeros(_lib.query("ka_arena_state_words", self.num_slots), dtype=torch.int32, device=dev)
            self._state_host = torch.zeros(self._state.shape, dtype=torch.int32).pin_memory()
            self._model_of = torch.full((N,), -1, dtype=torch.int32, device=dev)
            self._pre = torch.zeros(N, dtype=torch.uint8, device=dev)
            self._jobs = torch.zeros(self.num_slots, 4, dtype=torch.int32, device=dev)
            self._jobs_host = torch.zeros(self.num_slots, 4, dtype=torch.int32).pin_memory()
            self.collect = bool(collect)
            if self.collect:
                # one region of sync_every x envs_per_match rows per slot: a slot's rows of one chunk are a contiguous
                # slice and cannot overflow between two sync points
                S, cap = self.num_slots, self.sync_every * self.envs_per_match
                self._cap = cap
                self._bits = torch.zeros(S, dtype=torch.int32, device=dev)
                self._bits_host = torch.zeros(S, dtype=torch.int32).pin_memory()
                self._cursors = torch.zeros(_lib.query("ka_arena_cursor_words", S), dtype=torch.int32, device=dev)
                self._cursors_host = torch.zeros(self._cursors.shape, dtype=torch.int32).pin_memory()
                self._row_of = torch.full((N,), -1, dtype=torch.int32, device=dev)
                self._store = {"observations": torch.zeros(S * cap, 50, 9, 9, device=dev),
                               "legal_mask_bits": torch.zeros(S * cap, MASK_WORDS, dtype=torch.int32, device=dev),
                               "actions": torch.zeros(S * cap, dtype=torch.int64, device=dev),
                               "perspective": torch.zeros(S * cap, dtype=torch.uint8, device=dev),
                               "rewards": torch.zeros(S * cap, device=dev), "dones": torch.zeros(S * cap, device=dev)}
            self.features = bool(features)
            if self.features:
                # an env finishes at most one game per ply, so sync_every x envs_per_match records per slot cannot
                # overflow between two sync points
                S = self.num_slots
                accw, recw, curw = (_lib.query("ka_arena_feature_words", i) for i in range(3))
                self._fcap, self._fcurw = self.sync_every * self.envs_per_match, curw
                self._facc = torch.zeros(N * accw, dtype=torch.int32, device=dev)
                self._frecords = torch.zeros(S * self._fcap, recw, dtype=torch.int32, device=dev)
                self._frecords_host = torch.zeros(self._frecords.shape, dtype=torch.int32).pin_memory()
                self._fcursors = torch.zeros(S * curw, dtype=torch.int32, device=dev)
                self._fcursors_host = torch.zeros(self._fcursors.shape, dtype=torch.int32).pin_memory()
                every = torch.zeros(S, 4, dtype=torch.int32)
                every[:, 0] = torch.arange(S, dtype=torch.int32)
                self._every_slot = every.to(dev)                  # seat jobs naming every slot: the round-start clear
        self._graph: Optional[torch.cuda.CUDAGraph] = None

    def _set(self, option: str, controls) -> None:
        """New controls for ``option`` from the next ply on (between two ``run_round`` calls); nothing is captured again.
        None writes rows that are off (neutral rows for the sampler).  Refused: an arena built without the option -- its ply
        and its captured graph hold no launch of it --, ``collect=True``, a wrong row count and a size above the size built
        (``PlyStage.rewrite``)."""
        rewriters = {} if self._ctl is None else {"sampling": self._rewrite_sampling}
        for stage in self.ply.stages.values():
            rewriters.update(stage.rewriters())
        if option not in rewriters:
            raise ValueError(f"this arena was built without {option}=: its ply (and its captured graph) holds no launch of "
                             f"it; build the arena with {option}= controls to change them later")
        rewriters[option](controls, len(self.group), self.collect)

    def _rewrite_sampling(self, sampling, num_models: int, collect: bool) -> None:
        table = arena_controls(sampling, num_models, collect)
        with torch.cuda.device(self.device):
            self._ctl.copy_(torch.from_numpy(controls_table(None, num_models) if table is None else table))

    def set_sampling(self, sampling) -> None:
        self._set("sampling", sampling)

    def set_lookahead(self, lookahead) -> None:
        self._set("lookahead", lookahead)

    def set_search(self, search) -> None:
        self._set("search", search)

    def set_mcts(self, mcts) -> None:
        self._set("mcts", mcts)

    def set_mcts_explore(self, mcts_explore) -> None:
        self._set("mcts_explore", mcts_explore)

    def set_mate(self, mate) -> None:
        self._set("mate", mate)

    # ------------------------------------------------------------------ one ply
    def _ply(self) -> None:
        """forward -> sample -> step -> referee on the current stream; no host synchronisation."""
        ply = self.ply
        sp = self._state.data_ptr()
        cur, pre, _, _, st = ply.move(self._model_of, len(self.group), sp, sp + 4 * _SAMP)
        if self.collect:
            sto = self._store
            _lib.call("ka_arena_record_pre", self._state, self._bits, self.num_slots, self.envs_per_match, cur.observations,
                      cur.legal_mask_bits, self._actions, self._pre, self._nlegal, self._cursors, self._row_of,
                      sto["observations"], sto["legal_mask_bits"], sto["actions"], sto["perspective"], self._cap,
                      _OBS_ELEMS, MASK_WORDS, st)
        r = ply.step()
        if self.collect:
            _lib.call("ka_arena_record_post", self._cursors, self._row_of, self.num_slots, self.envs_per_match, r.rewards,
                      r.terminated, r.truncated, sto["rewards"], sto["dones"], self._cap, st)
        if self.features:                                 # before the referee: it rewrites status and pre_player
            meta = r.step_metadata
            _lib.call("ka_arena_features_step", self._state, self.num_slots, self.envs_per_match, self._actions, self._pre,
                      self._nlegal, meta.captured_piece, meta.termination_reason, meta.ply_count, r.rewards, r.terminated,
                      r.truncated, self._facc, self._frecords, self._fcursors, self._fcap, st)
        # before the referee: it rewrites model_of and the round ply
        ply.sample(r, pre, self._model_of, st)
        ply.log(r, pre, live=self._model_of, pairs=sp + 4 * _HDR, pair_stride=_SLOT, envs_per_pair=self.envs_per_match,
                ply_counter=sp + 4 * _PLY)
        # env._err[1] is the VecEnv's refusal latch: the referee copies it into the state so the host sees a refused
        # step in the same read
        _lib.call("ka_arena_referee", self._state, self.num_slots, self.envs_per_match, r.rewards,
                  r.terminated, r.truncated, r.current_players, self._nlegal, self.env._err.data_ptr() + 8, self._model_of,
                  self._pre, st)

    def _ply_recorded(self) -> None:
        cur = self.env.current()
        rec = {"seed": int(self._state[:2].view(torch.int64).item()), "obs": cur.observations.cpu(),
               "mask_bits": cur.legal_mask_bits.cpu(), "model_of": self._model_of.cpu(),
               "pre_players": self.env._players[self.env._cur].cpu(),
               "game_plies": self.env._state[:, GAME_PLY_BYTE:GAME_PLY_BYTE + 4].cpu().contiguous().view(torch.int32).reshape(-1)}
        self._ply()
        for stage in self.ply.stages.values():
            rec.update(stage.record())
        if self.search_samples is not None:
            rec.update(material_balance=self.env._material[self.env._cur].cpu())
        rec.update(actions=self._actions.cpu(), log_probs=self._logp.cpu(), n_legal=self._nlegal.cpu(),
                   rewards=self.env._rewards[self.env._cur].cpu(), terminated=self.env._terminated[self.env._cur].cpu(),
                   truncated=self.env._truncated[self.env._cur].cpu())
        if self.features:
            rec.update(captured_piece=self.env._captured[self.env._cur].cpu(),
                       termination_reason=self.env._reason[self.env._cur].cpu(),
                       ply_count=self.env._ply[self.env._cur].cpu().to(torch.int32) & 0xFFFF)    # a uint16 payload
        self.record.append(rec)

    def _chunk(self) -> None:
        if self._graph is not None:
            self._graph.replay()
            return
        for _ in range(self.sync_every):
            self._ply_recorded() if self.record_enabled else self._ply()

    def _capture(self) -> None:
        """Capture sync_every plies (after a warm-up ply pair on a side stream, which loads the kernels); the round that
        follows resets the env and the state, so the warm-up leaves nothing behind."""
        self.env.reset()
        s = torch.cuda.Stream(self.device)
        s.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(s):
            self._ply()
            self._ply()
        torch.cuda.current_stream(self.device).wait_stream(s)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(self.sync_every):
                self._ply()
        self._graph = g

    # ------------------------------------------------------------------ host side
    def _read_state(self) -> np.ndarray:
        if self.collect:                              # same stream: complete when the state copy below returns
            self._cursors_host.copy_(self._cursors, non_blocking=True)
        if self.features:
            self._fcursors_host.copy_(self._fcursors, non_blocking=True)
        self._state_host.copy_(self._state)           # the one device -> host read of a sync point
        st = self._state_host.numpy()
        if st[_SAMP]:
            raise RuntimeError("NaN in raw policy logits in MatchArena — probability tensor contains nan "
                               "(a model has diverged)")
        if st[_REFUSAL] or st[_REFUSAL + 1]:
            self.env.raise_if_refused()               # a refused step here is a bug: it raises
        return st

    def _assign(self, jobs: List[Tuple[int, int, int, int]], bits: Sequence[int] = ()) -> None:
        if not jobs:
            return
        if self.collect:
            for (s, _, _, _), b in zip(jobs, bits):
                self._bits_host[s] = b
            self._bits.copy_(self._bits_host, non_blocking=True)
        self._jobs_host[:len(jobs)] = torch.tensor(jobs, dtype=torch.int32)
        self._jobs.copy_(self._jobs_host, non_blocking=True)
        env = self.env
        _lib.call("ka_arena_assign", self._state, self._jobs, len(jobs), self.envs_per_match, env._players[env._cur],
                  self._model_of, self._pre, _lib.stream_ptr(self.device))
        if self.features:                                 # a new tracker per pairing (concurrent_matches.py:125)
            _lib.call("ka_arena_features_seat", self._jobs, len(jobs), self.num_slots, self.envs_per_match, self._facc,
                      _lib.stream_ptr(self.device))
        if self.game_log is not None:                     # the new pairing inherits the games in progress
            self.game_log.seat(self._jobs, len(jobs))

    def _drain(self, slot_pairing: Dict[int, int], chunks: Dict[int, list], lost: set) -> None:
        """Sync point: move the chunk's rows of every collecting slot out of the store (device to device) and reset the
        cursors.  The host has read only the cursor array."""
        cur = self._cursors_host.numpy().reshape(self.num_slots, _CUR)
        for s, p in slot_pairing.items():
            n = int(cur[s, 0])
            if cur[s, 2]:
                lost.add(p)
            if n:
                lo = s * self._cap
                chunks.setdefault(p, []).append({k: t[lo:lo + n].clone() for k, t in self._store.items()})
        self._cursors.zero_()

    def _drain_features(self, slot_pairing: Dict[int, int], games: Dict[int, list], stats: RoundStats) -> None:
        """Sync point: the chunk's game records of every slot that finished games come to the host (exactly the committed
        ones, one copy per such slot) and join their pairing's list; the cursors are reset."""
        cur = self._fcursors_host.numpy().reshape(self.num_slots, self._fcurw)
        stats.features_dropped += int(cur[:, 1].sum())
        took = []
        for s, p in slot_pairing.items():
            n = int(cur[s, 0])
            if n:
                lo = s * self._fcap
                self._frecords_host[lo:lo + n].copy_(self._frecords[lo:lo + n], non_blocking=True)
                took.append((p, lo, n))
        if took:
            torch.cuda.current_stream(self.device).synchronize()
            host = self._frecords_host.numpy()
            for p, lo, n in took:
                games.setdefault(p, []).append(host[lo:lo + n].copy())
        if cur.any():
            self._fcursors.zero_()

    def live_games(self, envs: Optional[Sequence[int]] = None) -> List[RecordedGame]:
        """The games in progress (every env, or ``envs``) between two rounds: ``RecordedGame`` with ``finished=False``,
        named by the models the env's slot holds now."""
        sp = self._state.data_ptr()
        return self.ply.live_games("an arena", envs, pairs=sp + 4 * _HDR, pair_stride=_SLOT,
                                   envs_per_pair=self.envs_per_match, ply_counter=sp + 4 * _PLY)

    def spectator_data(self, envs: Optional[Sequence[int]] = None) -> List[dict]:
        """``DevicePly.spectator_data`` between two rounds; ``insight`` is None before an env's first move of the round
        and for the envs of an idle slot."""
        return self.ply.spectator_data(envs)

    def run_round(self, pairings: Sequence[Tuple[int, int]], games_per_match: int = 64, *, max_ply: Optional[int] = None,
                  trainable: Union[None, Callable[[int, int], int], Mapping[int, int]] = None,
                  entry_ids: Union[None, Sequence[int], Mapping[int, int]] = None, epoch: int = 0):
        """Play every pairing ``(a, b)`` (model indices into the group, priority order) for ``games_per_match`` games.
        ``max_ply`` sets the ply ceiling ``max_ply * (ceil(games_per_match / envs_per_match) + 1)`` of a pairing, after
        which it ends with a partial result, as the reference's ``run_round(max_ply=)`` does (default: the env's max_ply).
        ``trainable`` (an arena built with ``collect=True``): a callable ``(a, b) -> bits`` or a mapping pairing index ->
        bits, bit 0 = collect the rows of side A, bit 1 = of side B; those pairings' results carry a ``MatchRollout``.
        ``entry_ids`` (model index -> league entry id; default: the model index) and ``epoch`` name the rows of the
        results' ``feature_tracker`` (an arena built with ``features=True``), as the reference's ``run_round(epoch=)``.
        Returns ``(results, stats)``: one MatchResult per pairing, in pairing order, and the round's RoundStats."""
        pairings = _check_round(pairings, games_per_match, len(self.group))
        if trainable is not None and not self.collect:
            raise ValueError("run_round(trainable=) needs an arena built with collect=True")
        bits = _side_bits(trainable, pairings)
        if entry_ids is not None:
            missing = sorted({m for pair in pairings for m in pair
                              if (m not in entry_ids if isinstance(entry_ids, Mapping) else m >= len(entry_ids))})
            if missing:
                raise ValueError(f"entry_ids names no id for models {missing}")
        max_ply = self.max_ply if max_ply is None else int(max_ply)
        if max_ply < 1:
            raise ValueError(f"max_ply must be positive, got {max_ply}")
        stats = RoundStats(pairings_requested=len(pairings))
        for stage in self.ply.stages.values():            # (every row off: nothing is searched, the counters stay 0)
            vars(stats).update(stage.fresh())
        if not pairings:
            return [], stats
        with torch.cuda.device(self.device), torch.no_grad():
            return self._run(pairings, int(games_per_match), max_ply, stats, bits, entry_ids, int(epoch))

    def _run(self, pairings, games_per_match, max_ply, stats, bits, entry_ids=None, epoch=0):
        if self.graph and self._graph is None:
            self._capture()
        t0 = time.monotonic()
        seed = self.seed if self.seed is not None else int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        hdr = torch.zeros(self._state.shape, dtype=torch.int32)
        hdr[:2].view(torch.int64)[0] = seed
        hdr[_MAX_PLY] = max_ply
        self._state.copy_(hdr)
        self._model_of.fill_(-1)
        if self.collect:
            self._cursors.zero_()
            self._bits_host.zero_()
        if self.features:
            self._fcursors.zero_()
            _lib.call("ka_arena_features_seat", self._every_slot, self.num_slots, self.num_slots, self.envs_per_match,
                      self._facc, _lib.stream_ptr(self.device))
        self.ply.reset()
        logged: Dict[int, List[RecordedGame]] = {}
        self.record = []
        chunks: Dict[int, list] = {}
        lost: set = set()
        games: Dict[int, list] = {}
        P = len(pairings)
        slot_pairing: Dict[int, int] = {}
        active: List[int] = []
        jobs = []
        nxt = 0
        for s in range(min(self.num_slots, P)):
            a, b = pairings[nxt]
            jobs.append((s, a, b, games_per_match))
            slot_pairing[s] = nxt
            active.append(s)
            nxt += 1
        stats.active_slots = len(active)
        self._assign(jobs, [bits[slot_pairing[j[0]]] for j in jobs])
        results: Dict[int, MatchResult] = {}
        while active:
            self._chunk()
            st = self._read_state()
            for stage in self.ply.stages.values():        # raises on its error word
                vars(stats).update(stage.read())
            stats.host_syncs += 1
            slot = st[_HDR:].reshape(self.num_slots, _SLOT)
            if self.collect:
                self._drain(slot_pairing, chunks, lost)
            if self.features:
                self._drain_features(slot_pairing, games, stats)
            if self.game_log is not None:                 # a slot's games of this chunk are its seated pairing's
                for g in self.game_log.drain():
                    logged.setdefault(slot_pairing[g.env // self.envs_per_match], []).append(g)
                stats.games_dropped = self.game_log.dropped
            jobs = []
            for i in sorted((i for i, s in enumerate(active) if slot[s, 7] & DONE), reverse=True):
                s = active.pop(i)
                ma, mb, _, aw, bw, dr, plies, status = (int(v) for v in slot[s])
                p = slot_pairing.pop(s)
                results[p] = MatchResult(ma, mb, aw, bw, dr, plies, bool(status & PARTIAL))
                if p in lost:
                    stats.rollouts_dropped += 1
                    chunks.pop(p, None)
                elif p in chunks:                           # to_result: the pairing's chunks become one rollout
                    parts = chunks.pop(p)
                    cat = {k: torch.cat([c[k] for c in parts]) for k in parts[0]}
                    results[p].rollout = MatchRollout(cat["observations"], cat["actions"], cat["rewards"], cat["dones"],
                                                      None, cat["perspective"], cat["legal_mask_bits"])
                    stats.rollout_rows += int(cat["actions"].shape[0])
                if self.features:
                    recs = games.pop(p, [])
                    recs = np.concatenate(recs) if recs else np.zeros((0, self._frecords.shape[1]), np.int32)
                    results[p].feature_tracker = GameFeatureTracker.from_records(
                        recs, _entry_id(entry_ids, ma), _entry_id(entry_ids, mb), epoch, self.envs_per_match)
                    stats.feature_rows += len(results[p].feature_tracker.completed_rows)
                if self.game_log is not None:
                    results[p].recorded_games = logged.pop(p, [])
                if nxt < P:
                    a, b = pairings[nxt]
                    jobs.append((s, a, b, games_per_match))
                    slot_pairing[s] = nxt
                    active.append(s)
                    nxt += 1
            self._assign(jobs, [bits[slot_pairing[j[0]]] for j in jobs])
        stats.round_plies = int(self._state_host[_PLY])
        stats.round_duration_s = time.monotonic() - t0
        ordered = [results[i] for i in range(P)]
        stats.pairings_completed = len(ordered)
        stats.total_games = sum(r.games for r in ordered)
        stats.total_plies = sum(r.plies for r in ordered)
        return ordered, stats
