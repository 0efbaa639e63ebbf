"""Search samples: the positions the arena's visit-count search looked at, kept inside the ply as training rows
(csrc/search_samples.hip; an addition the reference does not have).

``MctsSearch`` leaves a visit distribution over the root candidates for one ply, and the arena runs ``sync_every`` plies
under one captured graph, so no host code can read it in between.  ``SearchSamples`` is a store on the device that one
launch per ply (``ka_search_sample_step``, behind the env step and before the referee rewrites ``model_of``) writes: per
env a region of ``rows_per_env`` sample rows of 216 words -- the packed position (the 204 words of a ``DeviceSLDataset``
row: the observation before the move, the move played as policy, the value unlabelled, the material score), 8 visit words
``action | visits << 16`` and 4 info words ``model | mover << 16``, index of the move in its game, env, game number.  When
an env's game ends the same launch labels the game's rows W / D / L for their movers by the game log's rule.  ``drain()``
between two rounds appends the labelled rows, device to device, to a ``DeviceSLDataset`` with visit rows, which
``SLTrainer`` with ``visit_targets=True`` trains on.

``search_sample_step_host`` is the kernel in numpy over the same inputs -- the yardstick of the GPU tests;
``visit_words`` / ``unpack_visit_words`` restate the word format.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from keisei_amd import _lib
from keisei_amd.sl.dataset import NUM_ACTIONS, _RECORD
from keisei_amd.sl.device_dataset import INFO_WORDS, PACKED_WORDS, VISIT_SLOTS, DeviceSLDataset, pack_records, record_faults

from ._forked_rows import controls_rows
from .lookahead import FLAG_ACTIVE, REC_CAND, REC_FLAGS, REC_NCAND
from .mcts_search import MctsControls

__all__ = ["SearchSamples", "SearchSampleStats", "search_sample_step_host", "visit_words", "unpack_visit_words",
           "ROW_WORDS", "ROW_BYTES", "META_WORDS"]

VISIT_AT, INFO_AT = PACKED_WORDS, PACKED_WORDS + VISIT_SLOTS
ROW_WORDS = INFO_AT + INFO_WORDS                  # 216
ROW_BYTES = 4 * ROW_WORDS                         # 864
META_WORDS = 5
META_CURSOR, META_FIRST, META_DROPPED, META_MOVES, META_GAMES = range(META_WORDS)
ERR_UNPACKABLE = 1
_POLICY_AT = 200
_OBS_ELEMS = 4050


# ---------------------------------------------------------------------------------------------- the word format
def visit_words(actions, visits) -> np.ndarray:
    """The visit words ``uint32 (..., 8)`` of ``actions`` and ``visits`` (int, ``(..., w)`` with ``w <= 8``): word ``j`` is
    ``action | visits << 16`` where ``visits > 0`` and 0 elsewhere (an unused slot, and the slots behind ``w``)."""
    a, v = np.asarray(actions, np.int64), np.asarray(visits, np.int64)
    if a.shape != v.shape or a.ndim < 1 or a.shape[-1] > VISIT_SLOTS:
        raise ValueError(f"actions and visits are both (..., w) with w <= {VISIT_SLOTS}, got {a.shape} and {v.shape}")
    used = v > 0
    if used.any() and (a[used].min() < 0 or a[used].max() >= NUM_ACTIONS):
        raise ValueError(f"a visited slot's action must lie in [0, {NUM_ACTIONS})")
    if v.max(initial=0) > 0xFFFF:
        raise ValueError("visits must fit 16 bits")
    out = np.zeros(a.shape[:-1] + (VISIT_SLOTS,), np.uint32)
    out[..., :a.shape[-1]] = np.where(used, a | (v << 16), 0).astype(np.uint32)
    return out


def unpack_visit_words(words) -> Tuple[np.ndarray, np.ndarray]:
    """``(actions, visits)``, int32 ``(..., 8)`` each, of visit words: the action is -1 where the slot is unused."""
    w = np.asarray(words).astype(np.uint32, copy=False)
    visits = (w >> np.uint32(16)).astype(np.int32)
    return np.where(visits > 0, (w & np.uint32(0xFFFF)).astype(np.int32), -1).astype(np.int32), visits


# ---------------------------------------------------------------------------------------------- the kernel in numpy
def _np(x) -> np.ndarray:
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def search_sample_step_host(rows: np.ndarray, meta: np.ndarray, obs_prev, players_prev, records, root_visits, model_of,
                            actions, material, rewards, terminated, truncated) -> int:
    """``ka_search_sample_step`` in numpy: one ply over ``rows`` (uint32 ``(envs, rows_per_env, 216)``) and ``meta`` (int32
    ``(envs, 5)``), both written in place; returns the bits the launch ORs into the error word.  ``obs_prev`` (envs, 4050
    or 50 x 9 x 9, fp32) and ``players_prev`` are the env's buffers before the move, ``records`` (envs, 4 + 3 width) the
    search's records of simulation 0, ``root_visits`` (envs, width), ``actions`` the actions stepped, and ``material``,
    ``rewards``, ``terminated``, ``truncated`` the step's results."""
    E, R = rows.shape[0], rows.shape[1]
    assert rows.dtype == np.uint32 and rows.shape[2] == ROW_WORDS and meta.dtype == np.int32 and meta.shape == (E, META_WORDS)
    obs = np.ascontiguousarray(_np(obs_prev), np.float32).reshape(E, _OBS_ELEMS)
    pre = _np(players_prev).astype(np.int64).reshape(E) & 1
    rec = np.ascontiguousarray(_np(records)).view(np.int32).reshape(E, -1)
    vis = _np(root_visits).astype(np.int64).reshape(E, -1)
    W = vis.shape[1]
    mo, act = _np(model_of).astype(np.int64).reshape(E), _np(actions).astype(np.int64).reshape(E)
    mat, rew = _np(material).astype(np.int32).reshape(E), _np(rewards).astype(np.float32).reshape(E)
    done = _np(terminated).astype(bool).reshape(E) | _np(truncated).astype(bool).reshape(E)
    err = 0
    for e in range(E):
        cursor, first, dropped, moves, games = (int(x) for x in meta[e])
        ncand = int(rec[e, REC_NCAND])
        want = bool(rec[e, REC_FLAGS] & FLAG_ACTIVE) and ncand >= 1 and mo[e] >= 0
        fits = 0 <= cursor < R
        mover = int(pre[e])
        winner = mover if rew[e] > 0 else (1 - mover if rew[e] < 0 else 2)            # a NaN is a draw
        if want and fits:
            one = np.zeros(1, _RECORD)
            one["obs"], one["policy"], one["value"] = obs[e], act[e], -1
            one["score"] = np.float32(mat[e]) / np.float32(76.0)
            row = rows[e, cursor]
            row[:PACKED_WORDS] = pack_records(one)[0][0]
            if record_faults(one)[0][0]:
                err |= ERR_UNPACKABLE
            n = min(ncand, W)
            row[VISIT_AT:INFO_AT] = visit_words(rec[e, REC_CAND:REC_CAND + n], vis[e, :n])
            row[INFO_AT:] = (int(mo[e]) | (mover << 16), moves, e, games)
            if done[e]:
                row[_POLICY_AT + 1] = 1 if winner == 2 else (0 if winner == mover else 2)
        if done[e]:
            for r in range(max(first, 0), min(cursor, R)):
                m = int(rows[e, r, INFO_AT] >> 16) & 1
                rows[e, r, _POLICY_AT + 1] = 1 if winner == 2 else (0 if m == winner else 2)
        nxt = cursor + (1 if want and fits else 0)
        meta[e] = (nxt, nxt if done[e] else first, dropped + (1 if want and not fits else 0),
                   0 if done[e] else moves + 1, games + (1 if done[e] else 0))
    return err


def arena_search_samples(search_samples, mcts, num_models: int) -> int:
    """``MatchArena``'s reading of ``search_samples=``: the rows per env, 0 = off; refused without a visit-count search
    (``mcts=`` with a width above 0), whose visit counts the samples are."""
    if isinstance(search_samples, bool) or not isinstance(search_samples, (int, np.integer)) or search_samples < 0:
        raise ValueError(f"search_samples must be a non-negative integer (rows per env), got {search_samples!r}")
    if search_samples and (mcts is None or max(r.width for r in controls_rows(mcts, num_models, MctsControls, "mcts")) == 0):
        raise ValueError("search_samples needs mcts= with a width above 0: a sample is a searched position with the visit "
                         "counts of the visit-count search")
    return int(search_samples)


# ---------------------------------------------------------------------------------------------- the store
@dataclass
class SearchSampleStats:
    """What one ``drain()`` found in the store."""
    written: int = 0       # rows written since the store was last emptied
    labelled: int = 0      # of them: rows of finished games, handed to the dataset
    discarded: int = 0     # of them: rows of games still open, unlabelled, thrown away
    dropped: int = 0       # samples that found their env's region full and were never written


class SearchSamples:
    """The sample store of a device ``VecEnv`` under a visit-count search (``mcts``: its ``MctsSearch``):
    ``rows_per_env * envs * 864`` bytes, allocated here, once."""

    def __init__(self, env, mcts, rows_per_env: int) -> None:
        if isinstance(rows_per_env, bool) or not isinstance(rows_per_env, (int, np.integer)) or rows_per_env < 1:
            raise ValueError(f"rows_per_env must be a positive integer, got {rows_per_env!r}")
        if mcts is None:
            raise ValueError("search samples are the visit counts of a visit-count search: they need an MctsSearch")
        words = [_lib.query("ka_search_sample_words", i) for i in range(4)]
        if words != [ROW_WORDS, META_WORDS, VISIT_SLOTS, INFO_WORDS]:
            raise _lib.KeiseiHipError(f"libkeisei_amd.so lays a sample row out as {words}, keisei_amd.training.search_samples "
                                      f"as {[ROW_WORDS, META_WORDS, VISIT_SLOTS, INFO_WORDS]}: rebuild the library")
        if mcts.width > VISIT_SLOTS:
            raise ValueError(f"a sample row holds {VISIT_SLOTS} visit words, the search is {mcts.width} wide")
        self.env, self.mcts, self.rows_per_env = env, mcts, int(rows_per_env)
        n, dev = env.num_envs, env.device
        if n * self.rows_per_env > 2 ** 31 - 1:
            raise ValueError(f"{n} envs x {rows_per_env} rows: a store holds at most 2^31 - 1 rows")
        with torch.cuda.device(dev):
            self._rows = torch.zeros(n * self.rows_per_env, ROW_WORDS, dtype=torch.int32, device=dev)
            self._meta = torch.zeros(n * META_WORDS + 1, dtype=torch.int32, device=dev)      # the meta, then the error word
            self._meta_host = torch.zeros(self._meta.shape, dtype=torch.int32).pin_memory()

    @property
    def nbytes(self) -> int:
        return self._rows.numel() * 4

    def begin(self) -> None:
        """Zero the meta and the error word (the owner's reset): the rows of the games the reset abandons are gone."""
        self._meta.zero_()

    def step(self, obs_prev, players_prev, model_of, actions, material, rewards, terminated, truncated, stream) -> None:
        """The launch of one ply, behind the env step: ``obs_prev`` / ``players_prev`` the env's previous buffers."""
        mc, n = self.mcts, self.env.num_envs
        _lib.call("ka_search_sample_step", obs_prev, _OBS_ELEMS, players_prev, mc._records[0], int(mc._records.shape[2]),
                  mc._root_visits, mc.width, model_of, actions, material, rewards, terminated, truncated, self._rows,
                  self.rows_per_env, self._meta, self._meta.data_ptr() + 4 * n * META_WORDS, n, stream)

    # ------------------------------------------------------------------ host side
    def rows(self) -> torch.Tensor:
        """(envs, rows_per_env, 216) int32: a copy of the store on the device."""
        return self._rows.clone().reshape(self.env.num_envs, self.rows_per_env, ROW_WORDS)

    def meta(self) -> Tuple[torch.Tensor, int]:
        """``(meta (envs, 5) int32 on the host, error word)``: one device -> host read."""
        self._meta_host.copy_(self._meta)
        m = self._meta_host.clone()
        return m[:-1].reshape(self.env.num_envs, META_WORDS), int(m[-1])

    def drain(self, into: Optional[DeviceSLDataset] = None) -> Tuple[DeviceSLDataset, SearchSampleStats]:
        """Between two rounds: append the labelled rows, in (env, row) order and device to device, to ``into`` (or to a new
        ``DeviceSLDataset``) and empty the store.  One read of the meta.  The rows of games still open carry no label and
        are discarded; the move and game counters go on.  Raises on the error word."""
        n, R, dev = self.env.num_envs, self.rows_per_env, self.env.device
        if into is not None and torch.device(dev).index not in (None, into.device.index):
            raise ValueError(f"the dataset lives on {into.device}, the store on {dev}")
        with torch.cuda.device(dev):
            meta, err = self.meta()
            view = self._meta[:-1].view(n, META_WORDS)
            if err:
                self._meta[-1:].zero_()
                view[:, :META_MOVES].zero_()
                raise ValueError("Unpackable observation reached the search-sample store: channel values are not one-valued "
                                 "planes; the store has been emptied")
            m = meta.numpy().astype(np.int64)
            cursor = np.clip(m[:, META_CURSOR], 0, R)
            first = np.clip(m[:, META_FIRST], 0, cursor)
            stats = SearchSampleStats(int(cursor.sum()), int(first.sum()), int((cursor - first).sum()),
                                      int(m[:, META_DROPPED].sum()))
            dataset = DeviceSLDataset(dev) if into is None else into
            if stats.labelled:
                take = np.concatenate([e * R + np.arange(first[e]) for e in range(n) if first[e]])
                sel = self._rows.index_select(0, torch.from_numpy(take).to(dev))
                dataset.append_packed(sel[:, :PACKED_WORDS].contiguous(), sel[:, VISIT_AT:INFO_AT].contiguous(),
                                      sel[:, INFO_AT:].contiguous())
                dataset.check()
            view[:, :META_MOVES].zero_()
        return dataset, stats
