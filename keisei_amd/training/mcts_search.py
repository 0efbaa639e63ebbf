"""Visit-count (PUCT) search for the device ply: ``simulations`` forks of ``width`` rows per env, spread by
``Q + c P sqrt(N) / (1 + n)``, backed up as means, the most visited root candidate played.

The tree search of ``tree_search.py`` spends every fork on the leaf of the current principal variation and backs up by max and
negation, so one optimistic reading of the value head steers the whole budget, and all it hands back is a move and a line.
This search is what a policy-and-value network is built for: play that is robust to value noise and, per searched position, a
visit distribution over the root candidates (``MctsSearch.root_visits``, ``visit_policy``).  The node pool, the forks, the step
and the forward over a slice are the tree search's (``NodePool``); new is the tree policy, ``ka_mcts_advance``
(csrc/mcts.hip).  The reference never searches: the float64 restatement below is the meaning.

Semantics.  Row ``m`` of the controls table belongs to model ``m``: int32 ``width`` (0..8, 0 = off), fp32 ``c_puct`` (finite,
>= 0), int32 ``skip_plies`` -- read as the lookahead reads its row, and an env is active by the lookahead's rule -- and int32
``simulations`` (1..64; a word outside reads as 1, a value above the launch's is cut to it).  *Node* ``(t, j)`` is candidate
``j`` of simulation ``t`` (local node ``t * width + j``, pool row ``(t * envs + e) * width + j``) and keeps ``N`` (int32
visits), ``S`` (fp32 value sum for the player who moved into it), ``P`` (the fp32 prior the fork that created it wrote: priors
are used at every depth) and ``by`` (the simulation that forked it, -1 = never); a simulation keeps ``parent``, the node it
selected.  The root holds no statistics.  The leaf value ``q(t, j)`` is the tree search's (``search_leaf_q``), except that a
non-finite value logit of a live node -- an error -- makes it 0, so that no NaN enters a tree.

*Simulation 0* is the lookahead's fork of the env: every child gets ``N = 1``, ``S = q``.  *Selection* of simulation
``t >= 1``: from the root, at a node with children ``k``, ``Npar = sum N_k``, ``s_k = S_k / N_k`` plus ``c * P_k *
sqrtf(Npar) / (1 + N_k)`` when ``c > 0``, fp32 in that written order; the first maximum is chosen (ties keep the lower slot).
A chosen child that is live and was never forked is the *leaf*: it forks into slice ``t``.  A chosen child that is done or was
forked without a candidate is a *revisit*: nothing forks.  *Backup*: every new child gets ``N = 1``, ``S = q_k``; with
``v = max_k q_k`` the leaf gets ``N += 1, S += -v``, its parent ``N += 1, S += v``, the signs alternating up to the root's
child; a revisit (and a fork that found no candidate) adds the node's own ``q`` to it instead, alternating above.  One thread
adds, in simulation order: the order is part of the contract.  *Choice*: the root candidate of most visits (ties the lower
slot, the higher logit) replaces the sampler's action; where it differs from the arg-max of ``q(0, j)`` flag bit 3
(``MctsStats.deepened``) is set.  The *principal variation* is the chosen move, then the most visited child at each level down
to the first node never forked or done, padded with -1.
"""
from __future__ import annotations

import math
import struct
from dataclasses import dataclass
from typing import ClassVar, List, Optional, Tuple

import numpy as np
import torch

from keisei_amd import _lib
from keisei_amd.shogi_gym import ACTION_SPACE

from ._forked_rows import NodePool, PlyStage, check_int, check_weight, controls_rows, refuse_shared_place, table_of
from .lookahead import (FLAG_ACTIVE, MAX_SKIP_PLIES, MAX_WIDTH, REC_CAND, REC_FLAGS, REC_NCAND, _check_width, _row_controls,
                        lookahead_words)
from .mcts_explore import explore_table
from .sampling import GAME_PLY_BYTE
from .tree_search import node_record

__all__ = ["MctsControls", "MctsStats", "MctsTree", "MctsRestatement", "MctsSearch", "mcts_table", "mcts_simulations",
           "mcts_backup_select", "visit_policy", "arena_mcts", "MAX_SIMULATIONS"]

MAX_SIMULATIONS = 64


def _check_simulations(simulations, lo: int = 1) -> int:
    return check_int("simulations", simulations, lo, MAX_SIMULATIONS)


@dataclass(frozen=True)
class MctsControls:
    """One model's search controls.  ``width`` 0 is off; ``simulations`` 1 plays the most probable legal move."""
    width: int = 0
    simulations: int = 1
    c_puct: float = 0.0
    skip_plies: int = 0

    OFF: ClassVar["MctsControls"]

    def __post_init__(self) -> None:
        for name, hi in (("width", MAX_WIDTH), ("skip_plies", MAX_SKIP_PLIES)):
            object.__setattr__(self, name, check_int(name, getattr(self, name), 0, hi))
        object.__setattr__(self, "simulations", _check_simulations(self.simulations))
        object.__setattr__(self, "c_puct", check_weight("c_puct", self.c_puct))
        if self.simulations > 1 and self.width == 0:
            raise ValueError(f"simulations {self.simulations} needs a width above 0: there is no node to visit")

    def row(self) -> np.ndarray:
        """The table row: int32 width, fp32 c_puct, int32 skip_plies, int32 simulations, as four int32."""
        return np.frombuffer(struct.pack("<ifii", self.width, self.c_puct, self.skip_plies, self.simulations),
                             dtype=np.int32).copy()


MctsControls.OFF = MctsControls()


@dataclass
class MctsStats:
    """The counters ``ka_mcts_advance`` adds to."""
    searched: int = 0      # positions searched (active envs, summed over the plies)
    changed: int = 0       # choices that differ from the sampler's action
    won: int = 0           # chosen moves that ended the game as a win for the mover
    deepened: int = 0      # choices that differ from the arg-max of the root candidates' leaf q
    simulations: int = 0   # simulations run, summed over the envs and plies (simulation 0 included)
    revisits: int = 0      # of them: simulations that forked nothing and backed up the selected node's own q
    # the exploration's (``mcts_explore.py``; 0 for a search built without ``explore=True``)
    noised: int = 0        # positions whose root priors were noised
    sampled: int = 0       # moves drawn in proportion to the root visits
    diverged: int = 0      # of them: draws that differ from the most visited candidate


def _rows(controls, K) -> List[MctsControls]:
    return controls_rows(controls, K, MctsControls, "mcts")


def mcts_table(controls, K: int) -> np.ndarray:
    """The ``(K, 4)`` int32 table (``c_puct`` bit-cast).  ``controls``: None (K rows ``OFF``), one ``MctsControls`` (every
    model) or a sequence of exactly K."""
    return np.stack([r.row() for r in _rows(controls, K)]).astype(np.int32, copy=False)


def arena_mcts(mcts, num_models: int, collect: bool, lookahead=None, search=None) -> Tuple[Optional[np.ndarray], int, int]:
    """``MatchArena``'s reading of ``mcts=``: None stays None (the ply is what it was); everything else is a table of
    ``num_models`` rows, the largest width and the largest ``simulations`` in it -- refused together with ``lookahead=`` and
    ``search=`` (it stands where they stand) and with ``collect=True`` (a searched move is no draw from the policy)."""
    if mcts is None:
        return None, 0, 0
    refuse_shared_place(lookahead=lookahead, search=search, mcts=mcts)
    if collect:
        raise ValueError("a search cannot be combined with collect=True: DynamicTrainer treats the recorded actions as "
                         "draws from the entry's own policy, and a move chosen by the search is not one")
    rows = _rows(mcts, num_models)
    return mcts_table(rows, num_models), max(r.width for r in rows), max(r.simulations for r in rows)


def mcts_simulations(controls, model_of, *, simulations: int = MAX_SIMULATIONS):
    """Per row: ``(c_puct, simulations)`` as ``ka_mcts_advance`` reads them from the table: ``c_puct`` of a row that is on
    (else 0), word 3 outside [1, 64] or a model outside ``[0, K)`` reads as 1, a value above ``simulations`` (the launch's) is
    cut to it."""
    table = table_of(controls, None, mcts_table, "mcts")
    mo = np.asarray(torch.as_tensor(model_of).cpu().numpy(), np.int64).reshape(-1)
    cs, sims = np.zeros(mo.shape[0], np.float64), np.ones(mo.shape[0], np.int64)
    for b, m in enumerate(mo):
        if 0 <= m < table.shape[0]:
            cs[b] = _row_controls(table[m])[1]
            x = int(table[m, 3])
            sims[b] = min(x if 1 <= x <= MAX_SIMULATIONS else 1, int(simulations))
    return cs, sims


# ---------------------------------------------------------------------------------------------- the restatement
@dataclass
class MctsTree:
    """What the restatement holds for B rows after T simulations of width W."""
    N: np.ndarray           # (B, T, W) int: the visits (0 in the unused slots)
    S: np.ndarray           # (B, T, W) float64: the value sums, added in simulation order
    S32: np.ndarray         # (B, T, W) float32: the same sums added in fp32, the kernel's own arithmetic
    P: np.ndarray           # (B, T, W) float64: the priors (the records' fp32 values)
    by: np.ndarray          # (B, T, W) int: the simulation that forked the node (-1 = never), the next one included
    ran: np.ndarray         # (T, B) bool: simulation t ran for the row
    revisit: np.ndarray     # (T, B) bool: it forked nothing (or found no candidate) and backed up the selected node's own q
    slot: np.ndarray        # (T, B) int: the slot last selected among the children simulation t forked (-1: never)
    selections: list        # [t][b]: the selection of simulation t, a list of (x, scores (n,) float64, chosen slot) per
    #                         level, x the simulation whose children were scored; [] where none was made
    next_node: np.ndarray   # (B,) int: the local node simulation T selected, -1 = none (inactive or past simulations_m)
    fork_next: np.ndarray   # (B,) bool: it is a leaf and forks (else a revisit)
    choice: np.ndarray      # (B,) int: the root slot of most visits (-1 for an inactive row)
    one_ply: np.ndarray     # (B,) int: the arg-max over q(0, j)
    deepened: np.ndarray    # (B,) bool
    pv: np.ndarray          # (B, T) int: the principal variation's actions, padded with -1
    visits: np.ndarray      # (B, W) int: the root candidates' visits
    mean: np.ndarray        # (B, W) float64: their mean values S / N (0 in the unused slots)


def _first_max(values) -> int:
    best = 0
    for k in range(1, len(values)):
        if values[k] > values[best]:                           # ties keep the lower slot
            best = k
    return best


class MctsRestatement:
    """The float64 restatement of ``ka_mcts_advance``, one simulation per ``advance`` call, for B rows of width W and at
    most ``simulations`` simulations.  ``controls``: an ``MctsControls``, a sequence of them or a (K, 4) table; ``model_of``
    (B,) (default: model 0)."""

    def __init__(self, controls, model_of, B: int, W: int, simulations: int) -> None:
        self.B, self.W, self.E = int(B), int(W), int(simulations)
        mo = np.zeros(B, np.int64) if model_of is None else np.asarray(torch.as_tensor(model_of).cpu().numpy(), np.int64)
        self.c, self.sims = mcts_simulations(controls, mo)
        E, self.T = self.E, 0
        self.N = np.zeros((B, E, W), np.int64)
        self.S = np.zeros((B, E, W))
        self.S32 = np.zeros((B, E, W), np.float32)
        self.P = np.zeros((B, E, W))
        self.q = np.zeros((B, E, W))
        self.by = np.full((B, E, W), -1, np.int64)
        self.done = np.zeros((B, E, W), bool)
        self.cand = np.full((B, E, W), -1, np.int64)
        self.n_of = np.zeros((B, E), np.int64)
        self.parent = np.full((E, B), -1, np.int64)
        self.ran = np.zeros((E, B), bool)
        self.revisit = np.zeros((E, B), bool)
        self.slot = np.full((E, B), -1, np.int64)
        self.root = np.zeros(B, bool)
        self.selections: list = []
        self.next_node = np.full(B, -1, np.int64)
        self.fork_next = np.zeros(B, bool)

    def _select(self, b: int, t: int) -> list:
        """The selection of simulation ``t + 1`` for row b: sets ``next_node`` / ``fork_next``, returns its levels."""
        W, N, S, P, by = self.W, self.N[b].reshape(-1), self.S[b].reshape(-1), self.P[b].reshape(-1), self.by[b].reshape(-1)
        c, levels, x = float(self.c[b]), [], 0
        while True:
            n = int(self.n_of[b, x])
            n_par = int(N[x * W:x * W + n].sum())
            scores = np.zeros(n)
            for k in range(n):
                s = S[x * W + k] / N[x * W + k]
                if c > 0:
                    s = s + c * P[x * W + k] * math.sqrt(n_par) / (1 + N[x * W + k])
                scores[k] = s
            k = _first_max(scores)
            levels.append((x, scores, k))
            self.slot[x, b] = k
            node = x * W + k
            self.next_node[b] = node
            if self.done[b].reshape(-1)[node]:
                break                                          # the game ended there: a revisit
            if by[node] < 0:
                self.fork_next[b] = True                       # never forked and live: the leaf
                break
            if self.n_of[b, by[node]] == 0:
                break                                          # forked without a candidate: a revisit
            x = int(by[node])
        return levels

    def advance(self, records_t, done_t, parent_t=None, *, q=None) -> "MctsRestatement":
        """Simulation ``t`` (the next one): ``records_t`` (B, 4 + 3 W) int32 as the fork kernels and the advance wrote them
        (flags bit 0, n_cand, candidates, priors, leaf q), ``done_t`` (B, W) the new nodes' terminated-or-truncated flags,
        ``parent_t`` (B,) the local node the simulation selected (-1: it did not run; None: this restatement's own
        ``next_node``).  ``q`` (B, W) float64 replaces the record's fp32 leaf values."""
        t, B, W = self.T, self.B, self.W
        if t >= self.E:
            raise ValueError(f"the restatement was built for {self.E} simulations")
        rec = np.asarray(torch.as_tensor(records_t).cpu().numpy()).view(np.int32).reshape(B, lookahead_words(W))
        f = rec.view(np.float32)
        dn = np.asarray(torch.as_tensor(done_t).cpu().numpy()).astype(bool).reshape(B, W)
        par = self.next_node.copy() if parent_t is None else np.asarray(torch.as_tensor(parent_t).cpu().numpy(), np.int64).reshape(B)
        leaf = f[:, REC_CAND + 2 * W:REC_CAND + 3 * W].astype(np.float64) if q is None else np.asarray(q, np.float64).reshape(B, W)
        if t == 0:
            self.root = (rec[:, REC_FLAGS] & FLAG_ACTIVE) != 0
            par = np.full(B, -1, np.int64)
        self.parent[t] = np.where(self.root, par, -1) if t else -1
        self.next_node[:] = -1
        self.fork_next[:] = False
        sel = [[] for _ in range(B)]
        for b in range(B):
            if not self.root[b]:
                continue
            L = int(par[b])
            ran = t == 0 or 0 <= L < t * W
            if not ran:
                continue
            self.ran[t, b] = True
            N, S, S32, by = self.N[b].reshape(-1), self.S[b].reshape(-1), self.S32[b].reshape(-1), self.by[b].reshape(-1)
            forked = t == 0 or (not self.done[b].reshape(-1)[L] and by[L] in (-1, t))
            if t > 0 and forked:
                by[L] = t
            n = min(max(int(rec[b, REC_NCAND]), 1), W) if forked and rec[b, REC_FLAGS] & FLAG_ACTIVE else 0
            self.n_of[b, t] = n
            self.q[b, t, :n] = leaf[b, :n]
            self.N[b, t, :n] = 1
            self.S[b, t, :n] = leaf[b, :n]
            self.S32[b, t, :n] = leaf[b, :n].astype(np.float32)
            self.P[b, t, :n] = f[b, REC_CAND + W:REC_CAND + W + n]
            self.cand[b, t, :n] = rec[b, REC_CAND:REC_CAND + n]
            self.done[b, t, :n] = dn[b, :n]
            if t > 0:                                          # the backup: from the selected node to the root's child
                self.revisit[t, b] = n == 0
                val = self.q[b].reshape(-1)[L] if n == 0 else 0.0 - leaf[b, _first_max(leaf[b, :n])]
                node = L
                while True:
                    N[node] += 1
                    S[node] += val
                    S32[node] = np.float32(S32[node]) + np.float32(val)
                    if node < W:
                        break
                    node = int(self.parent[node // W, b])
                    val = 0.0 - val
            if t + 1 < self.sims[b]:
                sel[b] = self._select(b, t)
        self.selections.append(sel)
        self.T = t + 1
        return self

    def tree(self) -> MctsTree:
        """The tree after the simulations so far, with the choice, the flags and the line as the last launch takes them."""
        T, B, W = self.T, self.B, self.W
        by = self.by[:, :T].copy()
        for b in range(B):
            if self.fork_next[b]:
                by[b].reshape(-1)[self.next_node[b]] = T
        out = MctsTree(self.N[:, :T].copy(), self.S[:, :T].copy(), self.S32[:, :T].copy(), self.P[:, :T].copy(), by,
                       self.ran[:T].copy(), self.revisit[:T].copy(), self.slot[:T].copy(), [list(s) for s in self.selections],
                       self.next_node.copy(), self.fork_next.copy(), np.full(B, -1, np.int64), np.full(B, -1, np.int64),
                       np.zeros(B, bool), np.full((B, T), -1, np.int64), np.zeros((B, W), np.int64), np.zeros((B, W)))
        for b in range(B):
            if not self.root[b]:
                continue
            n = int(self.n_of[b, 0])
            N, done = self.N[b].reshape(-1), self.done[b].reshape(-1)
            out.visits[b, :n] = self.N[b, 0, :n]
            out.mean[b, :n] = self.S[b, 0, :n] / self.N[b, 0, :n]
            best = out.choice[b] = _first_max(self.N[b, 0, :n])
            out.one_ply[b] = _first_max(self.q[b, 0, :n])
            out.deepened[b] = out.choice[b] != out.one_ply[b]
            node, line = int(best), [int(self.cand[b, 0, best])]
            while len(line) < T and not done[node]:
                x = int(self.by[b].reshape(-1)[node])
                if x < 0 or x >= T or self.n_of[b, x] == 0:
                    break
                k = _first_max(N[x * W:x * W + int(self.n_of[b, x])])
                line.append(int(self.cand[b, x, k]))
                node = x * W + k
            out.pv[b, :len(line)] = line
        return out


def mcts_backup_select(records, done, parent, controls, model_of=None, *, q=None) -> MctsTree:
    """The float64 restatement of ``ka_mcts_advance`` after T simulations.  ``records`` (T, B, 4 + 3 W) int32 as the fork
    kernels and the advance wrote them (the kernel's own fp32 priors and leaf q), ``done`` (T, B, W) the nodes'
    terminated-or-truncated flags, ``parent`` (T, B) the local node ``t' * W + j`` simulation t selected (-1: simulation 0, or
    a simulation that did not run for the row), ``controls`` an ``MctsControls``, a sequence of them or a (K, 4) table and
    ``model_of`` (B,) (default: model 0).  ``q`` (T, B, W) float64 replaces the records' fp32 leaf values."""
    rec = np.asarray(torch.as_tensor(records).cpu().numpy()).view(np.int32)
    T, B = rec.shape[:2]
    W = (rec.shape[2] - REC_CAND) // 3
    dn = np.asarray(torch.as_tensor(done).cpu().numpy()).astype(bool).reshape(T, B, W)
    par = np.asarray(torch.as_tensor(parent).cpu().numpy(), np.int64).reshape(T, B)
    r = MctsRestatement(controls, model_of, B, W, MAX_SIMULATIONS)
    for t in range(T):
        r.advance(rec[t], dn[t], par[t], q=None if q is None else np.asarray(q, np.float64).reshape(T, B, W)[t])
    return r.tree()


def visit_policy(candidates, visits, temperature: float = 1.0) -> torch.Tensor:
    """The dense ``(envs, 11259)`` float32 policy target of a searched ply: ``visits ** (1 / temperature)`` normalised over
    the row's candidates, one-hot on the most visited candidate (ties the lower slot: the choice) at ``temperature`` 0, and a
    row of zeros for an env without a candidate.  ``candidates`` (envs, width) int (-1 = unused) and ``visits`` (envs, width)
    int as ``MctsSearch.root_visits`` gives them.  Torch code on the tensors' device, not on the ply's path."""
    if isinstance(temperature, bool) or not isinstance(temperature, (int, float)) or not math.isfinite(temperature) or temperature < 0:
        raise ValueError(f"temperature must be finite and >= 0, got {temperature!r}")
    cand, vis = torch.as_tensor(candidates).to(torch.int64), torch.as_tensor(visits)
    if cand.dim() != 2 or cand.shape != vis.shape:
        raise ValueError(f"candidates and visits are both (envs, width), got {tuple(cand.shape)} and {tuple(vis.shape)}")
    vis = vis.to(cand.device)
    used = (cand >= 0) & (cand < ACTION_SPACE) & (vis > 0)
    if bool(((vis > 0) & ~used).any()):
        raise ValueError("a visited slot names no action of the spatial action space")
    v = torch.where(used, vis, torch.zeros_like(vis)).double()
    if temperature == 0:
        w = torch.zeros_like(v)
        w.scatter_(1, v.argmax(1, keepdim=True), 1.0)          # (argmax takes the first maximum)
        w = w * used
    else:
        w = torch.where(used, (v / v.max(1, keepdim=True).values.clamp_min(1.0)) ** (1.0 / float(temperature)), torch.zeros_like(v))
    total = w.sum(1, keepdim=True)
    w = torch.where(total > 0, w / total.clamp_min(1e-300), torch.zeros_like(w))
    out = torch.zeros(cand.shape[0], ACTION_SPACE, dtype=torch.float32, device=cand.device)
    out.scatter_add_(1, torch.where(used, cand, torch.zeros_like(cand)), w.float())
    return out


# ---------------------------------------------------------------------------------------------- in the ply
class MctsSearch(NodePool):
    """The node pool of a device ``VecEnv`` (``NodePool``: ``simulations`` slices of ``envs * width`` rows and one scratch),
    the trees and the stages of the visit-count search.  Everything is allocated here, once.  ``explore=True`` also allocates
    what the exploration of ``mcts_explore.py`` writes: the raw priors, eta and three more counters."""

    _WORDS, _WHAT, _SLICE = "ka_mcts_words", "the visit-count search", "simulation"

    def __init__(self, env, group, width: int, simulations: int, explore: bool = False) -> None:
        width = _check_width(width)
        self.simulations = simulations = _check_simulations(simulations)
        assert width <= _lib.query("ka_mcts_words", 3, 0, 0) == MAX_WIDTH
        assert simulations <= _lib.query("ka_mcts_words", 4, 0, 0) == MAX_SIMULATIONS
        self._nexplore = _lib.query("ka_mcts_words", 7, width, simulations) if explore else 0
        super().__init__(env, group, width, simulations, extra_counters=self._nexplore)    # the exploration's counters
        assert self.words == lookahead_words(width) and self.tree_words == simulations + 4 * simulations * width
        n, dev = env.num_envs, env.device
        with torch.cuda.device(dev):
            self._root_visits = torch.zeros(n, width, dtype=torch.int32, device=dev)
            self._root_values = torch.zeros(n, width, dtype=torch.float32, device=dev)
            self._raw_priors = self._eta = None
            if explore:
                self._raw_priors = torch.zeros(n, width, dtype=torch.float32, device=dev)
                self._eta = torch.zeros(n, width, dtype=torch.float64, device=dev)

    def advance(self, t: int, actions, model_of, table, stream, explore_table=None, seed=None) -> None:
        """After ``evaluate(t)``: leaf q, backup, the selection of simulation t + 1; at the last simulation the choice --
        with ``explore_table`` and ``seed`` (``step``) the choice of ``ka_mcts_advance_explore``."""
        self.rows(t)
        args = (self._records, self._tree, self.width, self.simulations, t, table, model_of, int(table.shape[0]),
                self.value_logits, self.rewards, self.terminated, self.truncated, self._step_err, actions, self.parent_row,
                self.active, self._pv, self._root_visits, self._root_values, self._counters,
                self._counters.data_ptr() + 4 * self._nstats)
        if explore_table is None:
            _lib.call("ka_mcts_advance", *args, self.env.num_envs, stream)
        else:
            env = self.env
            _lib.call("ka_mcts_advance_explore", *args, explore_table, seed, env._state.data_ptr() + GAME_PLY_BYTE,
                      env._state.shape[1], self._explore_stats(), env.num_envs, stream)

    def _explore_stats(self) -> int:
        if not self._nexplore:
            raise ValueError("the exploration needs an MctsSearch built with explore=True")
        return self._counters.data_ptr() + 4 * (self._nstats + 1)

    def root_noise_step(self, model_of, explore_table, seed, stream) -> None:
        """Behind ``fork`` and before ``advance(0)``: ``ka_mcts_root_noise`` over the records of simulation 0."""
        _lib.call("ka_mcts_root_noise", self._records[0], self.width, explore_table, model_of, int(explore_table.shape[0]),
                  seed, self._raw_priors, self._eta, self._explore_stats(), self.env.num_envs, stream)

    def step(self, logits, mask_bits, actions, model_of, table, stream, explore_table=None, seed=None) -> None:
        """``NodePool.step``.  With ``explore_table`` (the (K, 4) int32 table of ``mcts_explore.py`` on the device) and
        ``seed`` (the device pointer of the int64 the ply's sampler reads) the root noise is launched behind the fork of
        simulation 0 and the advance is ``ka_mcts_advance_explore``; without them the launches are what they were."""
        if explore_table is None:
            return super().step(logits, mask_bits, actions, model_of, table, stream)
        if seed is None:
            raise ValueError("explore_table= needs seed=, the device pointer of the ply's sampler seed")
        for t in range(self.slices):
            if t == 0:
                self.fork(logits, mask_bits, actions, model_of, table, stream)
                self.root_noise_step(model_of, explore_table, seed, stream)
            else:
                self.expand(t, table, stream)
            self.step_nodes(t, stream)
            self.evaluate(t)
            self.advance(t, actions, model_of, table, stream, explore_table, seed)

    # ------------------------------------------------------------------ host side
    def read(self) -> MctsStats:
        """At a sync point: the counters since ``clear()`` (one small device -> host copy).  Raises on the error word."""
        c = self._read_counters()
        return MctsStats(*(int(v) for v in c[:6]), *(int(v) for v in c[self._nstats + 1:self._nstats + 4][:self._nexplore]))

    def tree(self) -> dict:
        """The trees of the last ``step`` (copies on the device): ``parent`` (envs, simulations) int32, and (envs,
        simulations, width) each ``N`` int32, ``S`` fp32, ``P`` fp32 and ``by`` int32."""
        E, W, n = self.simulations, self.width, self.env.num_envs
        t = self._tree.clone()
        part = lambda i: t[:, E + i * E * W:E + (i + 1) * E * W]  # noqa: E731
        return {"parent": t[:, :E], "N": part(0).reshape(n, E, W), "S": part(1).view(torch.float32).reshape(n, E, W),
                "P": part(2).view(torch.float32).reshape(n, E, W), "by": part(3).reshape(n, E, W)}

    def root_noise(self) -> Tuple[torch.Tensor, torch.Tensor]:
        """``(raw_priors, eta)`` of the last ``step`` with an exploration table (copies on the device), (envs, width) each:
        the root priors before the noise (fp32) and the Dirichlet draw (float64), 0 in the unused slots.  The kernel writes
        the rows it noises and no other: a row not noised in the last ply keeps what an earlier ply left (0 at first)."""
        if self._eta is None:
            raise ValueError("root_noise() needs an MctsSearch built with explore=True")
        return self._raw_priors.clone(), self._eta.clone()

    def root_visits(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """``(candidates, visits, mean_values)`` of the last ``step`` (copies on the device), (envs, width) each: the root
        candidates' actions (int32, -1 = unused or an inactive env), their visits (int32) and their mean values ``S / N``
        (fp32) for the player to move.  ``visit_policy`` makes a dense target of the first two."""
        rec0 = self._records[0]
        active = (rec0[:, REC_FLAGS] & FLAG_ACTIVE).ne(0)[:, None]
        cand = torch.where(active, rec0[:, REC_CAND:REC_CAND + self.width], torch.full_like(rec0[:, :1], -1))
        return cand, self._root_visits.clone(), self._root_values.clone()


class MctsStage(PlyStage):
    """The visit-count search as a loop builds it into its ply (``mcts=``: an ``MctsControls`` for every model, or one per
    model), where the lookahead stands.  The node pool is sized by the largest ``width`` and ``simulations`` given;
    ``set_mcts`` goes up to them.  ``engine.root_visits()`` between two plies gives the visit distribution of every searched
    position, ``RoundStats.mcts`` carries the counters.  The stage owns the exploration of ``mcts_explore.py``
    (``mcts_explore=``): its table (None: nothing is allocated and the launches are those of the search alone), the
    ``explore=`` flag of the engine and ``set_mcts_explore``; ``engine.root_noise()`` gives the priors before the noise and
    the draw, ``RoundStats.mcts`` the counters ``noised`` / ``sampled`` / ``diverged``."""

    name, shares_place, STATS = "mcts", True, MctsStats
    _ROWS = "node pool's rows"

    def __init__(self, table: np.ndarray, explore: Optional[np.ndarray] = None, **sizes: int) -> None:
        super().__init__(table, **sizes)
        self.host_explore_table, self.explore_table = explore, None

    @classmethod
    def parse(cls, mcts, num_models: int, collect: bool, explore: Optional[np.ndarray] = None) -> Optional["MctsStage"]:
        """``explore``: the exploration table as ``arena_mcts_explore`` read it."""
        table, width, simulations = arena_mcts(mcts, num_models, collect)
        if table is None and explore is not None:
            raise ValueError("an exploration needs mcts=: it is the visit-count search that is explored")
        return None if table is None else cls(table, explore, width=width, simulations=simulations)

    @classmethod
    def _off(cls, num_models: int) -> "MctsStage":
        return cls(mcts_table(None, num_models), width=0, simulations=1)

    def build(self, env, group) -> None:
        super().build(env, group)
        if self.host_explore_table is not None:
            self.explore_table = torch.from_numpy(self.host_explore_table).to(env.device)

    def _engine(self, env, group) -> Optional[MctsSearch]:
        if not self.sizes["width"]:
            return None
        return MctsSearch(env, group, **self.sizes, explore=self.host_explore_table is not None)

    def _launch(self, logits, mask_bits, actions, model_of, seed, stream) -> None:
        # (with an exploration the noise and the drawn move read the sampler's seed of this ply)
        self.engine.step(logits, mask_bits, actions, model_of, self.table, stream, explore_table=self.explore_table, seed=seed)

    def rewriters(self) -> dict:
        explore = {} if self.explore_table is None else {"mcts_explore": self.rewrite_explore}
        return dict(super().rewriters(), **explore)

    def rewrite_explore(self, mcts_explore, num_models: int, collect: bool) -> None:
        """New exploration controls from the next ply on; nothing is captured again.  None writes rows that are off: the
        games are then those of the search alone."""
        with torch.cuda.device(self.explore_table.device):
            self.explore_table.copy_(torch.from_numpy(explore_table(mcts_explore, num_models)))

    def _record(self) -> dict:
        mc = self.engine
        rec = dict(node_record(mc, "mcts"), mcts_root_visits=tuple(x.cpu() for x in mc.root_visits()))
        if self.explore_table is not None:
            rec.update(mcts_root_noise=tuple(x.cpu() for x in mc.root_noise()))
        return rec
