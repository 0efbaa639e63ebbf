"""Tree search for the device ply: best-first minimax over ``expansions`` forks of ``width`` rows per env.

The lookahead of ``lookahead.py`` searches one ply, its reply search two, at ``width * reply_width`` rows per env.  A forked
row after ``ka_shogi_env_step`` is a complete env row and the forward over the forked rows writes their policy logits anyway,
so a deeper search needs only a tree: remember every node, spend each new batch of ``width`` rows on the leaf of the current
principal variation, back the values up.  ``expansions = E`` and ``width = W`` evaluate ``E * W`` rows per env and follow the
best line up to ``E`` plies deep.  The reference never searches: the float64 restatement below is the meaning.

Semantics.  Row ``m`` of the controls table belongs to model ``m``: int32 ``width`` (0..8), fp32 ``prior_weight``, int32
``skip_plies`` -- read exactly as the lookahead reads them, and an env is active by the lookahead's rule -- and int32
``expansions`` (1..16; a word outside reads as 1).  *Expansion 0* is the lookahead's fork of the env: candidates, priors and
one child per candidate.  *Node* ``(t, j)`` is candidate ``j`` of expansion ``t`` (local node ``t * width + j``).  Its leaf
value ``q(t, j)`` is for the player who moved into it: the env's reward of that step where the game ended there, else
``P(L) - P(W)`` of ``softmax(value_logits)`` of the env's model on the node's observation; a non-finite value logit of a live
node makes it -inf and is an error.  *Backed-up value*: ``val(n) = q(n)`` for a node never expanded or whose expansion found
no candidate, else ``0 - max_k val(child k)``, the first maximum over the node's candidates.  *Principal leaf*: at the root
the first maximum of ``u_j = val(0, j) + prior_weight * p_j`` (``val`` alone at weight 0), below it the first maximum of
``val`` over the node's children (priors below the root are recorded and not used); descend until the node is done or was
expanded without a candidate -- the env's search is finished and it is inactive in every later expansion -- or is unexpanded:
the leaf.  *Expansion* ``t``, ``1 <= t < expansions_m``, forks the leaf's first ``width_m`` legal moves by the node's own
logits in the candidate order; the children carry the node's full history and are stepped and evaluated like any row.
*Choice*: after the last expansion the first maximum of ``u_j`` at the root replaces the sampler's action; the one-ply choice
is the same arg-max over ``q(0, j)``, and a row where the two differ sets flag bit 3 (``SearchStats.deepened``).  The
*principal variation* is the chosen move, then the first-maximum children down to the first unexpanded or done node, at most
``expansions`` actions, padded with -1.  Values back up by max and negation only, which are exact in fp32: the one rounded
operation is the root's ``q + prior_weight * prior``.  ``expansions = 1`` is the one-ply lookahead bit for bit.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass
from typing import ClassVar, List, Optional, Tuple

import numpy as np
import torch

from keisei_amd import _lib
from keisei_amd.shogi_gym import ACTION_SPACE

from ._forked_rows import (ERR_VALUE, NodePool, PlyStage, check_int, check_weight, controls_rows, refuse_shared_place,
                           table_of)
from .lookahead import (FLAG_ACTIVE, MAX_SKIP_PLIES, MAX_WIDTH, REC_CAND, REC_FLAGS, REC_NCAND, _check_width,
                        _loss_minus_win, _row_controls, lookahead_words)

__all__ = ["SearchControls", "SearchStats", "SearchTree", "TreeSearch", "search_table", "search_expansions", "search_records",
           "search_leaf_q", "search_backup_select", "arena_search", "MAX_EXPANSIONS", "FLAG_DEEPENED"]

MAX_EXPANSIONS = 16
FLAG_DEEPENED = 8


def _check_expansions(expansions, lo: int = 1) -> int:
    return check_int("expansions", expansions, lo, MAX_EXPANSIONS)


@dataclass(frozen=True)
class SearchControls:
    """One model's search controls.  ``width`` 0 is off; ``expansions`` 1 is the one-ply lookahead."""
    width: int = 0
    expansions: int = 1
    prior_weight: float = 0.0
    skip_plies: int = 0

    OFF: ClassVar["SearchControls"]

    def __post_init__(self) -> None:
        for name, hi in (("width", MAX_WIDTH), ("skip_plies", MAX_SKIP_PLIES)):
            object.__setattr__(self, name, check_int(name, getattr(self, name), 0, hi))
        object.__setattr__(self, "expansions", _check_expansions(self.expansions))
        object.__setattr__(self, "prior_weight", check_weight("prior_weight", self.prior_weight))
        if self.expansions > 1 and self.width == 0:
            raise ValueError(f"expansions {self.expansions} needs a width above 0: there is no node to expand")

    def row(self) -> np.ndarray:
        """The table row: int32 width, fp32 prior_weight, int32 skip_plies, int32 expansions, as four int32."""
        return np.frombuffer(struct.pack("<ifii", self.width, self.prior_weight, self.skip_plies, self.expansions),
                             dtype=np.int32).copy()


SearchControls.OFF = SearchControls()


@dataclass
class SearchStats:
    """The counters ``ka_search_advance`` adds to."""
    searched: int = 0      # positions searched (active envs, summed over the plies)
    changed: int = 0       # choices that differ from the sampler's action
    won: int = 0           # chosen moves that ended the game as a win for the mover
    deepened: int = 0      # choices that differ from the one-ply choice
    expansions: int = 0    # expansions run, summed over the envs and plies (expansion 0 included)


def _rows(controls, K) -> List[SearchControls]:
    return controls_rows(controls, K, SearchControls, "search")


def search_table(controls, K: int) -> np.ndarray:
    """The ``(K, 4)`` int32 table (the weight bit-cast).  ``controls``: None (K rows ``OFF``), one ``SearchControls`` (every
    model) or a sequence of exactly K."""
    return np.stack([r.row() for r in _rows(controls, K)]).astype(np.int32, copy=False)


def arena_search(search, num_models: int, collect: bool, lookahead=None) -> Tuple[Optional[np.ndarray], int, int]:
    """``MatchArena``'s reading of ``search=``: None stays None (the ply is what it was); everything else is a table of
    ``num_models`` rows, the largest width and the largest ``expansions`` in it -- refused together with ``lookahead=`` (the
    search stands where the lookahead stands) and with ``collect=True`` (a searched move is no draw from the policy)."""
    if search is None:
        return None, 0, 0
    refuse_shared_place(lookahead=lookahead, search=search)
    if collect:
        raise ValueError("a search cannot be combined with collect=True: DynamicTrainer treats the recorded actions as "
                         "draws from the entry's own policy, and a move chosen by the search is not one")
    rows = _rows(search, num_models)
    return search_table(rows, num_models), max(r.width for r in rows), max(r.expansions for r in rows)


def search_expansions(controls, model_of, *, expansions: int = MAX_EXPANSIONS):
    """Per row: ``(prior_weight, expansions)`` as ``ka_search_advance`` reads them from the table: the weight of a row that
    is on (else 0), word 3 outside [1, 16] or a model outside ``[0, K)`` reads as 1, a value above ``expansions`` (the
    launch's) is cut to it."""
    table = table_of(controls, None, search_table, "search")
    mo = np.asarray(torch.as_tensor(model_of).cpu().numpy(), np.int64).reshape(-1)
    weights, exps = np.zeros(mo.shape[0], np.float64), np.ones(mo.shape[0], np.int64)
    for b, m in enumerate(mo):
        if 0 <= m < table.shape[0]:
            weights[b] = _row_controls(table[m])[1]
            x = int(table[m, 3])
            exps[b] = min(x if 1 <= x <= MAX_EXPANSIONS else 1, int(expansions))
    return weights, exps


# ---------------------------------------------------------------------------------------------- the restatement
def search_records(n_cand, priors=None, q=None, cands=None) -> torch.Tensor:
    """Records ``(T, B, 4 + 3 width)`` int32 as the kernels lay them out, from ``n_cand`` (T, B), ``priors`` and ``q``
    (T, B, width) (default 0) and ``cands`` (T, B, width) int (default: candidate j is "action" ``t * width + j``)."""
    n_cand = np.asarray(n_cand, np.int64)
    T, B = n_cand.shape
    width = (np.asarray(q).shape[2] if q is not None else np.asarray(priors).shape[2])
    rec = np.zeros((T, B, lookahead_words(width)), np.int32)
    rec[:, :, REC_FLAGS] = n_cand > 0
    rec[:, :, REC_NCAND] = n_cand
    used = np.arange(width)[None, None, :] < n_cand[:, :, None]
    if cands is None:
        cands = np.broadcast_to((np.arange(T)[:, None, None] * width + np.arange(width)[None, None, :]), (T, B, width))
    rec[:, :, REC_CAND:REC_CAND + width] = np.where(used, np.asarray(cands, np.int64), -1)
    f = rec.view(np.float32)
    if priors is not None:
        f[:, :, REC_CAND + width:REC_CAND + 2 * width] = np.where(used, np.asarray(priors, np.float32), 0)
    if q is not None:
        f[:, :, REC_CAND + 2 * width:REC_CAND + 3 * width] = np.where(used, np.asarray(q, np.float32), 0)
    return torch.from_numpy(rec)


def search_leaf_q(value_logits, rewards, done) -> Tuple[np.ndarray, int]:
    """The leaf values in float64 and the error word: ``value_logits`` (..., 3), ``rewards`` and ``done`` (...)."""
    vl = np.asarray(torch.as_tensor(value_logits).double().numpy())
    rw = np.asarray(torch.as_tensor(rewards).double().numpy())
    dn = np.asarray(torch.as_tensor(done).numpy()).astype(bool)
    q = np.zeros(rw.shape, np.float64)
    error = 0
    for i in np.ndindex(*rw.shape):
        if dn[i]:
            q[i] = rw[i]
        elif not np.isfinite(vl[i]).all():
            q[i] = -np.inf
            error |= ERR_VALUE
        else:
            q[i] = _loss_minus_win(vl[i])
    return q, error


@dataclass
class SearchTree:
    """What ``search_backup_select`` returns for B rows after T expansions of width W."""
    val: np.ndarray         # (B, T, W) float64: the backed-up values (0 in the unused slots)
    by: np.ndarray          # (B, T, W) int: the expansion that forked the node (-1 = never), the next one included
    slot: np.ndarray        # (T, B) int: the first-maximum child of the node expansion t forked (-1: it has no candidate)
    u: np.ndarray           # (B, W) float64: val(0, j) + prior_weight * prior (-inf in the unused slots)
    next_node: np.ndarray   # (B,) int: the local node expansion T forks, -1 = none (inactive, finished or past expansions_m)
    finished: np.ndarray    # (B,) bool: the principal line ends in a done node or one expanded without a candidate
    choice: np.ndarray      # (B,) int: the first maximum of u (-1 for an inactive row)
    one_ply: np.ndarray     # (B,) int: the same arg-max over q(0, j)
    deepened: np.ndarray    # (B,) bool
    pv: np.ndarray          # (B, T) int: the principal variation's actions, padded with -1


def search_backup_select(records, done, parent, controls, model_of=None, *, q=None) -> SearchTree:
    """The float64 restatement of ``ka_search_advance`` after T expansions.  ``records`` (T, B, 4 + 3 W) int32 as the fork
    kernels and the advance wrote them (flags bit 0, n_cand, candidates, priors, leaf q), ``done`` (T, B, W) the nodes'
    terminated-or-truncated flags, ``parent`` (T, B) the local node ``t' * W + j`` that expansion t forked (-1: expansion 0,
    or an expansion that did not run for the row), ``controls`` a ``SearchControls``, a sequence of them or a (K, 4) table and
    ``model_of`` (B,) (default: model 0).  ``q`` (T, B, W) float64 replaces the records' fp32 leaf values."""
    rec = np.asarray(torch.as_tensor(records).cpu().numpy()).view(np.int32)
    T, B = rec.shape[:2]
    W = (rec.shape[2] - REC_CAND) // 3
    dn = np.asarray(torch.as_tensor(done).cpu().numpy()).astype(bool).reshape(T, B, W)
    par = np.asarray(torch.as_tensor(parent).cpu().numpy(), np.int64).reshape(T, B)
    mo = np.zeros(B, np.int64) if model_of is None else np.asarray(torch.as_tensor(model_of).cpu().numpy(), np.int64)
    weights, exps = search_expansions(controls, mo)
    f = rec.view(np.float32)
    prior = f[0, :, REC_CAND + W:REC_CAND + 2 * W].astype(np.float64)
    leaf = f[:, :, REC_CAND + 2 * W:REC_CAND + 3 * W].astype(np.float64) if q is None else np.asarray(q, np.float64).reshape(T, B, W)
    out = SearchTree(np.zeros((B, T, W)), np.full((B, T, W), -1, np.int64), np.full((T, B), -1, np.int64),
                     np.full((B, W), -np.inf), np.full(B, -1, np.int64), np.zeros(B, bool), np.full(B, -1, np.int64),
                     np.full(B, -1, np.int64), np.zeros(B, bool), np.full((B, T), -1, np.int64))
    for b in range(B):
        root = bool(rec[0, b, REC_FLAGS] & FLAG_ACTIVE)
        if not root:
            continue
        pw = float(weights[b])
        val, by, slot = out.val[b].reshape(-1), out.by[b].reshape(-1), out.slot[:, b]
        n_of = [0] * T

        def u_of(j, v):
            return v + pw * prior[b, j] if pw > 0 else v

        def first_max(x):
            best = 0
            for k in range(n_of[x]):
                vk = u_of(k, val[k]) if x == 0 else val[x * W + k]
                vb = u_of(best, val[best]) if x == 0 else val[x * W + best]
                if vk > vb:                                    # ties keep the lower slot
                    best = k
            return best

        for t in range(T):
            ran = t == 0 or par[t, b] >= 0
            n = min(max(int(rec[t, b, REC_NCAND]), 1), W) if ran and rec[t, b, REC_FLAGS] & FLAG_ACTIVE else 0
            n_of[t] = n
            val[t * W:t * W + n] = leaf[t, b, :n]
            if t > 0 and ran:
                by[par[t, b]] = t
            x = t
            while n > 0:                                       # the backup: from the forked node to the root
                slot[x] = first_max(x)
                if x == 0:
                    break
                p = int(par[x, b])
                val[p] = 0.0 - val[x * W + slot[x]]
                x = p // W
        for j in range(n_of[0]):
            out.u[b, j] = u_of(j, val[j])
        out.choice[b] = slot[0]
        best1 = 0
        for k in range(n_of[0]):
            if u_of(k, leaf[0, b, k]) > u_of(best1, leaf[0, b, best1]):
                best1 = k
        out.one_ply[b] = best1
        out.deepened[b] = best1 != slot[0]
        # the principal line
        node, line = int(slot[0]), [int(rec[0, b, REC_CAND + slot[0]])]
        while True:
            if dn.reshape(T * B * W)[(node // W * B + b) * W + node % W]:
                out.finished[b] = True
                break
            x = int(by[node])
            if x < 0:
                if T < exps[b]:
                    out.next_node[b] = node
                break
            if n_of[x] == 0:
                out.finished[b] = True
                break
            line.append(int(rec[x, b, REC_CAND + slot[x]]))
            node = x * W + int(slot[x])
        if out.next_node[b] >= 0:
            by[out.next_node[b]] = T
        out.pv[b, :len(line)] = line[:T]
    return out


# ---------------------------------------------------------------------------------------------- in the ply
class TreeSearch(NodePool):
    """The node pool of a device ``VecEnv`` (``NodePool``: ``expansions`` slices of ``envs * width`` rows and one scratch) and
    the stages of the search.  Everything is allocated once.  Slice ``t`` of the pool is rows ``[t * envs * width, (t + 1) *
    envs * width)``; node ``(t, j)`` of env ``e`` is row ``(t * envs + e) * width + j``."""

    _WORDS, _WHAT, _SLICE = "ka_search_words", "the search", "expansion"

    def __init__(self, env, group, width: int, expansions: int) -> None:
        width = _check_width(width)
        self.expansions = expansions = _check_expansions(expansions)
        assert width <= _lib.query("ka_search_words", 3, 0, 0) == MAX_WIDTH
        assert expansions <= _lib.query("ka_search_words", 4, 0, 0) == MAX_EXPANSIONS
        super().__init__(env, group, width, expansions)
        assert self.words == lookahead_words(width) and self.tree_words == expansions + 2 * expansions * width

    # ------------------------------------------------------------------ the stages
    def advance(self, t: int, actions, model_of, table, stream) -> None:
        """After ``evaluate(t)``: leaf q, backup, the leaf of expansion t + 1; at the last expansion the choice."""
        self.rows(t)
        _lib.call("ka_search_advance", self._records, self._tree, self.width, self.expansions, t, table, model_of,
                  int(table.shape[0]), self.value_logits, self.rewards, self.terminated, self.truncated, self._step_err,
                  actions, self.parent_row, self.active, self._pv, self._counters,
                  self._counters.data_ptr() + 4 * self._nstats, self.env.num_envs, stream)

    # ------------------------------------------------------------------ host side
    def read(self) -> SearchStats:
        """At a sync point: the counters since ``clear()`` (one small device -> host copy).  Raises on the error word."""
        return SearchStats(*(int(v) for v in self._read_counters()[:5]))

    def tree(self) -> dict:
        """The trees of the last ``step`` (copies on the device): ``parent`` (envs, expansions) int32, ``val`` (envs,
        expansions, width) fp32 and ``by`` (envs, expansions, width) int32."""
        E, W, n = self.expansions, self.width, self.env.num_envs
        t = self._tree.clone()
        return {"parent": t[:, :E], "val": t[:, E:E + E * W].view(torch.float32).reshape(n, E, W),
                "by": t[:, E + E * W:].reshape(n, E, W)}


def node_record(pool: NodePool, prefix: str) -> dict:
    """What a recorded ply keeps of a node pool's last ``step``: the records, the trees and the lines under ``prefix``, the
    pool's rows under ``node_*``, (slices, envs, width) each."""
    shape = (pool.slices, pool.env.num_envs, pool.width)
    return {f"{prefix}_records": pool.records().cpu(), f"{prefix}_tree": {k: v.cpu() for k, v in pool.tree().items()},
            f"{prefix}_pv": pool.principal_variations().cpu(), "node_value_logits": pool.value_logits.cpu().reshape(*shape, 3),
            "node_rewards": pool.rewards.cpu().reshape(shape),
            "node_done": (pool.terminated | pool.truncated).cpu().reshape(shape),
            "node_logits": pool.logits.cpu().reshape(-1, ACTION_SPACE), "node_mask_bits": pool.mask_bits.cpu(),
            "node_model_of": pool.model_of.cpu().reshape(shape)}


class SearchStage(PlyStage):
    """The tree search as a loop builds it into its ply (``search=``: a ``SearchControls`` for every model, or one per
    model), where the lookahead stands.  The node pool is sized by the largest ``width`` and ``expansions`` given;
    ``set_search`` goes up to them.  ``RoundStats.search`` carries the counters."""

    name, shares_place, STATS = "search", True, SearchStats
    _ROWS = "node pool's rows"

    @classmethod
    def parse(cls, search, num_models: int, collect: bool) -> Optional["SearchStage"]:
        table, width, expansions = arena_search(search, num_models, collect)
        return None if table is None else cls(table, width=width, expansions=expansions)

    @classmethod
    def _off(cls, num_models: int) -> "SearchStage":
        return cls(search_table(None, num_models), width=0, expansions=1)

    def _engine(self, env, group) -> Optional[TreeSearch]:
        return TreeSearch(env, group, **self.sizes) if self.sizes["width"] else None

    def _launch(self, logits, mask_bits, actions, model_of, seed, stream) -> None:
        self.engine.step(logits, mask_bits, actions, model_of, self.table, stream)

    def _record(self) -> dict:
        return node_record(self.engine, "search")
