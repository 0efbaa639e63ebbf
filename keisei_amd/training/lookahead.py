"""One-ply value lookahead for the device ply, per model.

Every move of ``MatchArena`` is one draw from the raw policy: an agent that walks past mates in one and hangs pieces.  A
game's complete state on the device is a few rows (a 128-byte state row plus ``ply`` words of key / check history) and the
grouped forward evaluates thousands of boards of mixed models in three launches, so a one-ply search is four stages on one
stream: ``ka_lookahead_fork`` (csrc/lookahead.hip: candidates, priors, one child row per candidate), the env's own
``ka_shogi_env_step`` over the child rows, the group's own forward over the child observations, and
``ka_lookahead_choose``.  The reference has nothing like it: it never searches.

Semantics (the float64 restatement below is the documented meaning).  Row ``m`` of the controls table belongs to model
``m``: ``width`` (0..8, 0 = the model plays the sampler's action), ``prior_weight`` (finite, >= 0) and ``skip_plies`` (the
lookahead leaves a position whose game ply is below it to the sampler, so an opening schedule of ``SamplingControls`` still
diversifies openings).  A row with ``width`` outside [0, 8], a negative or non-finite weight or a negative ``skip_plies``
reads as off.  Env ``e`` with model ``m = model_of[e]`` is *active* when ``m`` lies in ``[0, K)``, ``width_m > 0``, its game
ply is ``>= skip_plies_m`` and it has a candidate.  *Candidates*: the first ``width_m`` legal actions by raw logit descending,
equal logits by lower action (the order of the policy insight and the sampling controls); a legal logit that is -inf or NaN
is never a candidate.  *Prior* ``p_j``: the candidate's softmax probability over all legal actions at temperature 1, the row
maximum subtracted (a NaN logit weighs nothing).  *Child* ``j``: the position after candidate ``j``, with the env's full
history behind it, decided exactly as ``ka_shogi_env_step`` decides it.  ``q_j`` is the env's reward for the mover when the
child is terminated or truncated, else ``P(L) - P(W)`` of ``softmax(value_logits_j)`` of model ``m`` on the child's
observation (the child is seen by its side to move); a non-finite value logit of a live child is an error and makes ``q_j``
-inf.  The choice is the first ``j`` of the greatest ``u_j = q_j + prior_weight_m * p_j``; an active env plays candidate
``j``, an inactive env keeps the sampler's action, and nothing else about the ply changes.
"""
from __future__ import annotations

import math
import struct
from dataclasses import dataclass
from typing import ClassVar, Optional, Tuple

import numpy as np
import torch

from keisei_amd import _lib
from keisei_amd.shogi_gym import ACTION_SPACE, MASK_WORDS

__all__ = ["LookaheadControls", "LookaheadStats", "LookaheadChoice", "Lookahead", "lookahead_table", "lookahead_active",
           "lookahead_candidates", "lookahead_choose", "lookahead_words", "arena_lookahead", "MAX_WIDTH", "MAX_SKIP_PLIES"]

MAX_WIDTH = 8
MAX_SKIP_PLIES = 65535
# record words (csrc/lookahead.hip; ka_lookahead_words reports the sizes)
REC_FLAGS, REC_SLOT, REC_NCAND, REC_ACTION, REC_CAND = 0, 1, 2, 3, 4
FLAG_ACTIVE, FLAG_CHANGED, FLAG_WON = 1, 2, 4
ERR_VALUE, ERR_CHILD_STEP = 1, 2


def lookahead_words(width: int) -> int:
    """32-bit words of one record."""
    return REC_CAND + 3 * int(width)


@dataclass(frozen=True)
class LookaheadControls:
    """One model's lookahead controls.  ``width`` 0 is off."""
    width: int = 0
    prior_weight: float = 0.0
    skip_plies: int = 0

    OFF: ClassVar["LookaheadControls"]

    def __post_init__(self) -> None:
        for name, hi in (("width", MAX_WIDTH), ("skip_plies", MAX_SKIP_PLIES)):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 0 <= v <= hi:
                raise ValueError(f"{name} must be an integer in [0, {hi}], got {v!r}")
            object.__setattr__(self, name, int(v))
        w = self.prior_weight
        if isinstance(w, bool) or not isinstance(w, (int, float)) or not math.isfinite(w) or w < 0:
            raise ValueError(f"prior_weight must be finite and >= 0, got {w!r}")
        object.__setattr__(self, "prior_weight", float(w))
        if self.prior_weight > 3.0e38:
            raise ValueError(f"prior_weight must fit a float32 (at most 3.0e38), got {w!r}")

    def row(self) -> np.ndarray:
        """The table row: int32 width, fp32 prior_weight, int32 skip_plies, 0, as four int32."""
        return np.frombuffer(struct.pack("<ifii", self.width, self.prior_weight, self.skip_plies, 0), dtype=np.int32).copy()


LookaheadControls.OFF = LookaheadControls()


@dataclass
class LookaheadStats:
    """The counters ``ka_lookahead_choose`` adds to."""
    searched: int = 0      # positions searched (active envs, summed over the plies)
    changed: int = 0       # choices that differ from the sampler's action
    won: int = 0           # chosen moves that ended the game as a win for the mover


def _rows(controls, K: int):
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or K < 1:
        raise ValueError(f"a lookahead table needs at least one row, got K = {K!r}")
    K = int(K)
    if controls is None:
        return [LookaheadControls.OFF] * K
    if isinstance(controls, LookaheadControls):
        return [controls] * K
    if isinstance(controls, (list, tuple)):
        rows = list(controls)
        if len(rows) != K:
            raise ValueError(f"expected {K} LookaheadControls (one per model), got {len(rows)}")
        for r in rows:
            if not isinstance(r, LookaheadControls):
                raise ValueError(f"every entry must be a LookaheadControls, got {type(r).__name__}")
        return rows
    raise ValueError(f"lookahead must be None, a LookaheadControls or a sequence of {K}, got {type(controls).__name__}")


def lookahead_table(controls, K: int) -> np.ndarray:
    """The ``(K, 4)`` int32 table (the weight bit-cast).  ``controls``: None (K rows ``OFF``), one ``LookaheadControls``
    (every model) or a sequence of exactly K."""
    return np.stack([r.row() for r in _rows(controls, K)]).astype(np.int32, copy=False)


def arena_lookahead(lookahead, num_models: int, collect: bool) -> Tuple[Optional[np.ndarray], int]:
    """``MatchArena``'s reading of ``lookahead=``: None stays None (the ply is what it was); everything else is a table of
    ``num_models`` rows and the largest width in it -- refused with ``collect=True``, where ``DynamicTrainer`` treats the
    recorded actions as draws from the entry's own policy, which a searched move is not."""
    if lookahead is None:
        return None, 0
    if collect:
        raise ValueError("a lookahead cannot be combined with collect=True: DynamicTrainer treats the recorded actions as "
                         "draws from the entry's own policy, and a move chosen by the lookahead is not one")
    rows = _rows(lookahead, num_models)
    return lookahead_table(rows, num_models), max(r.width for r in rows)


def _table_of(controls, K: Optional[int]) -> np.ndarray:
    if isinstance(controls, torch.Tensor):
        controls = controls.detach().cpu().numpy()
    if isinstance(controls, np.ndarray):              # a table as it lies in device memory: taken as it is
        if controls.dtype != np.int32 or controls.ndim != 2 or controls.shape[1] != 4 or controls.shape[0] < 1:
            raise ValueError(f"a lookahead table is a (K, 4) int32 array, got {controls.dtype} {controls.shape}")
        if K is not None and controls.shape[0] != K:
            raise ValueError(f"expected a table of {K} rows, got {controls.shape[0]}")
        return np.ascontiguousarray(controls)
    if K is None:
        K = len(controls) if isinstance(controls, (list, tuple)) else 1
    return lookahead_table(controls, K)


def _row_controls(row: np.ndarray) -> Tuple[int, float, int]:
    """(width, prior_weight, skip_plies) of a table row as the kernels read it: a row with width outside [0, 8], a negative
    or non-finite weight or a negative skip_plies is off."""
    w, s = int(row[0]), int(row[2])
    pw = float(row[1:2].view(np.float32)[0])
    if not (0 <= w <= MAX_WIDTH and math.isfinite(pw) and pw >= 0 and s >= 0):
        return 0, 0.0, 0
    return w, pw, s


def lookahead_active(controls, model_of, plies=None, *, num_models: Optional[int] = None, width: int = MAX_WIDTH):
    """Per row: ``(width, prior_weight)`` as the kernels read them from the table -- width 0 for a row whose model lies
    outside ``[0, K)``, whose table row is off or invalid, or whose game ply is below ``skip_plies``; a width above
    ``width`` (the launch's) is cut to it.  ``plies`` None = past every ``skip_plies``.  (A row with a positive width is
    active when it also has a candidate.)"""
    table = _table_of(controls, num_models)
    mo = np.asarray(torch.as_tensor(model_of).cpu().numpy(), np.int64).reshape(-1)
    pl = None if plies is None else np.asarray(torch.as_tensor(plies).cpu().numpy(), np.int64).reshape(-1)
    widths, weights = np.zeros(mo.shape[0], np.int64), np.zeros(mo.shape[0], np.float64)
    for b, m in enumerate(mo):
        if not 0 <= m < table.shape[0]:
            continue
        w, pw, skip = _row_controls(table[m])
        if pl is not None and (pl[b] & 0xFFFFFFFF) < skip:
            w = 0
        widths[b], weights[b] = min(w, int(width)), pw
    return widths, weights


# ---------------------------------------------------------------------------------------------- candidates
def _check_width(width) -> int:
    if isinstance(width, bool) or not isinstance(width, (int, np.integer)) or not 1 <= width <= MAX_WIDTH:
        raise ValueError(f"width must be an integer in [1, {MAX_WIDTH}], got {width!r}")
    return int(width)


def lookahead_candidates(logits: torch.Tensor, legal: torch.Tensor, width: int):
    """``(candidates (B, width) int32, priors (B, width), n_cand (B,) int32)`` of B rows: the first ``width`` legal actions
    by raw logit descending, equal logits by lower action (-1 = unused), and their softmax probabilities over all legal
    actions.  ``logits`` (B, 11259) or (B, 9, 9, 139), fp32 or bf16; ``legal`` bool rows or packed int32 rows (B, 352).  CUDA
    tensors go through ``ka_lookahead_fork``; CPU tensors through the float64 restatement (priors in float64)."""
    width = _check_width(width)
    if logits.dim() < 2 or logits.shape[0] < 1:
        raise ValueError(f"logits must have shape (B, {ACTION_SPACE}) or (B, 9, 9, 139) with B >= 1, got {tuple(logits.shape)}")
    B = int(logits.shape[0])
    if logits.numel() != B * ACTION_SPACE:
        raise ValueError(f"the lookahead covers the spatial action space only ({ACTION_SPACE} actions), got {logits.numel() // B}")
    if logits.dtype not in (torch.float32, torch.bfloat16, torch.float64):
        raise ValueError(f"logits must be float32 or bfloat16, got {logits.dtype}")
    if legal.dtype == torch.bool and legal.numel() == B * ACTION_SPACE:
        packed = False
    elif legal.dtype == torch.int32 and tuple(legal.shape) == (B, MASK_WORDS):
        packed = True
    else:
        raise ValueError(f"legal must be bool (B, {ACTION_SPACE}) or packed int32 (B, {MASK_WORDS}), "
                         f"got {legal.dtype} {tuple(legal.shape)}")
    if logits.is_cuda:
        return _candidates_device(logits.reshape(B, ACTION_SPACE), legal, width, B, packed)
    return _candidates_host(logits.reshape(B, ACTION_SPACE), legal, width, B, packed)


def _candidates_device(logits, legal, width, B, packed):
    dev = logits.device
    with torch.cuda.device(dev):
        st = _lib.stream_ptr(dev)
        lg = (logits.float() if logits.dtype == torch.float64 else logits).contiguous()
        if packed:
            bits = legal.to(dev).contiguous()
        else:
            bits = torch.zeros(B, MASK_WORDS, dtype=torch.int32, device=dev)
            _lib.call("ka_pack_mask_bits", legal.reshape(B, ACTION_SPACE).to(dev).contiguous(), bits, B, ACTION_SPACE, st)
        table = torch.from_numpy(lookahead_table(LookaheadControls(width), 1)).to(dev)
        rec = torch.zeros(B, lookahead_words(width), dtype=torch.int32, device=dev)
        _lib.call("ka_lookahead_fork", lg, int(lg.dtype == torch.bfloat16), bits, MASK_WORDS,
                  torch.zeros(B, dtype=torch.int64, device=dev), torch.zeros(B, dtype=torch.int32, device=dev), 1, table,
                  None, None, None, 0, width, rec, None, None, None, None, None, None, B, ACTION_SPACE, st)
    return (rec[:, REC_CAND:REC_CAND + width], rec.view(torch.float32)[:, REC_CAND + width:REC_CAND + 2 * width],
            rec[:, REC_NCAND])


def _unpack(legal: torch.Tensor, B: int, packed: bool) -> np.ndarray:
    if not packed:
        return legal.reshape(B, ACTION_SPACE).numpy()
    j = np.arange(ACTION_SPACE)
    return ((legal.numpy().view(np.uint32)[:, j // 32] >> (j % 32).astype(np.uint32)) & 1).astype(bool)


def _candidates_host(logits, legal, width, B, packed):
    """The candidates and priors of ``ka_lookahead_fork`` in float64."""
    x = logits.double().numpy()
    mask = _unpack(legal, B, packed)
    cands = np.full((B, width), -1, np.int32)
    priors = np.zeros((B, width), np.float64)
    n_cand = np.zeros(B, np.int32)
    for b in range(B):
        idx = np.flatnonzero(mask[b])                                  # ascending action order
        if idx.size == 0:
            continue
        z = x[b, idx]
        key = np.where(np.isnan(z), -np.inf, z)
        order = np.argsort(-key, kind="stable")[:width]                # logit descending, equal logits by lower action
        order = order[key[order] > -np.inf]
        if order.size == 0:
            continue
        with np.errstate(over="ignore", invalid="ignore"):
            e = np.where(np.isnan(z), 0.0, np.exp(key - key.max()))
        n_cand[b] = order.size
        cands[b, :order.size] = idx[order]
        priors[b, :order.size] = e[order] / e.sum()
    return torch.from_numpy(cands), torch.from_numpy(priors), torch.from_numpy(n_cand)


# ---------------------------------------------------------------------------------------------- the choice
@dataclass
class LookaheadChoice:
    slot: torch.Tensor          # (B,)  int32: the chosen slot; -1 for a row without a candidate
    q: torch.Tensor             # (B, width): the children's values for the mover (0 in the unused slots)
    u: torch.Tensor             # (B, width): q + prior_weight * prior (-inf in the unused slots); host path fp64, device fp32
    error: int                  # bit 0: a non-finite value logit of a live child


def lookahead_choose(priors: torch.Tensor, n_cand: torch.Tensor, child_value_logits: torch.Tensor,
                     child_rewards: torch.Tensor, child_done: torch.Tensor, prior_weight) -> LookaheadChoice:
    """The choice of B rows.  ``priors`` (B, width), ``n_cand`` (B,), ``child_value_logits`` (B, width, 3),
    ``child_rewards`` (B, width) the env's rewards for the mover, ``child_done`` (B, width) terminated or truncated,
    ``prior_weight`` a float or one per row.  CUDA tensors go through ``ka_lookahead_choose``; CPU tensors through the
    float64 restatement."""
    if priors.dim() != 2 or not 1 <= priors.shape[1] <= MAX_WIDTH or priors.shape[0] < 1:
        raise ValueError(f"priors must have shape (B, width) with B >= 1 and width in [1, {MAX_WIDTH}], got {tuple(priors.shape)}")
    B, width = (int(s) for s in priors.shape)
    if n_cand.numel() != B or tuple(child_value_logits.shape) != (B, width, 3) or tuple(child_rewards.shape) != (B, width) \
            or tuple(child_done.shape) != (B, width):
        raise ValueError(f"expected n_cand ({B},), child_value_logits ({B}, {width}, 3), child_rewards and child_done "
                         f"({B}, {width})")
    pw = prior_weight.detach().cpu().numpy() if isinstance(prior_weight, torch.Tensor) else prior_weight
    pw = np.broadcast_to(np.asarray(pw, np.float64).reshape(-1), (B,)).copy()
    if not (np.isfinite(pw).all() and (pw >= 0).all()):
        raise ValueError("prior_weight must be finite and >= 0")
    if priors.is_cuda:
        return _choose_device(priors, n_cand, child_value_logits, child_rewards, child_done, pw, B, width)
    return _choose_host(priors, n_cand, child_value_logits, child_rewards, child_done, pw, B, width)


def _choose_host(priors, n_cand, vlogits, rewards, done, pw, B, width) -> LookaheadChoice:
    """The semantics of ``ka_lookahead_choose`` in float64."""
    p = priors.double().numpy()
    nc = np.clip(n_cand.reshape(B).numpy().astype(np.int64), 0, width)
    vl = vlogits.double().numpy()
    rw = rewards.double().numpy()
    dn = done.numpy().astype(bool)
    slot = np.full(B, -1, np.int32)
    q = np.zeros((B, width), np.float64)
    u = np.full((B, width), -np.inf, np.float64)
    error = 0
    for b in range(B):
        for j in range(int(nc[b])):
            if dn[b, j]:
                q[b, j] = rw[b, j]
            elif not np.isfinite(vl[b, j]).all():
                q[b, j] = -np.inf
                error |= ERR_VALUE
            else:
                e = np.exp(vl[b, j] - vl[b, j].max())
                q[b, j] = (e[2] - e[0]) / e.sum()                     # P(L) - P(W): the child is seen by its side to move
            u[b, j] = q[b, j] + pw[b] * p[b, j] if pw[b] > 0 else q[b, j]
            if j == 0 or u[b, j] > u[b, slot[b]]:                     # ties keep the lower slot
                slot[b] = j
    return LookaheadChoice(torch.from_numpy(slot), torch.from_numpy(q), torch.from_numpy(u), error)


def _choose_device(priors, n_cand, vlogits, rewards, done, pw, B, width) -> LookaheadChoice:
    dev = priors.device
    with torch.cuda.device(dev):
        W = lookahead_words(width)
        rec = torch.zeros(B, W, dtype=torch.int32, device=dev)
        nc = n_cand.reshape(B).to(device=dev, dtype=torch.int32).clamp(0, width)
        rec[:, REC_FLAGS] = (nc > 0).int()
        rec[:, REC_NCAND] = nc
        rec[:, REC_CAND:REC_CAND + width] = torch.arange(width, dtype=torch.int32, device=dev)      # candidate j = "action" j
        rec.view(torch.float32)[:, REC_CAND + width:REC_CAND + 2 * width] = priors.to(device=dev, dtype=torch.float32)
        # one table row per row of the batch: each carries its own weight
        table = torch.zeros(B, 4, dtype=torch.int32, device=dev)
        table[:, 0] = width
        table.view(torch.float32)[:, 1] = torch.from_numpy(pw.astype(np.float32)).to(dev)
        actions = torch.full((B,), -1, dtype=torch.int64, device=dev)
        stats = torch.zeros(_lib.query("ka_lookahead_words", 2, width), dtype=torch.int32, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        dn = done.to(device=dev, dtype=torch.uint8).contiguous()
        _lib.call("ka_lookahead_choose", rec, width, table, torch.arange(B, dtype=torch.int32, device=dev), B,
                  vlogits.to(device=dev, dtype=torch.float32).contiguous(), rewards.to(device=dev, dtype=torch.float32).contiguous(),
                  dn, torch.zeros_like(dn), None, actions, stats, err, B, _lib.stream_ptr(dev))
        q = rec.view(torch.float32)[:, REC_CAND + 2 * width:REC_CAND + 3 * width]
        used = torch.arange(width, device=dev)[None, :] < nc[:, None]
        w32 = table.view(torch.float32)[:, 1:2]
        u = torch.where(used, torch.where(w32 > 0, q + w32 * priors.to(device=dev, dtype=torch.float32), q),
                        torch.full_like(q, float("-inf")))
        slot = torch.where(nc > 0, rec[:, REC_SLOT], torch.full_like(nc, -1))
        return LookaheadChoice(slot, q, u, int(err.item()))


# ---------------------------------------------------------------------------------------------- in the ply
class Lookahead:
    """The child rows of a device ``VecEnv``, the second forward workspace and the four stages of the lookahead.
    Everything is allocated here, once: ``width`` child rows per env, each a state row, a key / check history row, two
    packed mask rows, the step's outputs and a row of the group's workspace.  ``records()`` (envs, 4 + 3 width) int32 are
    the envs' records of the last ``step``."""

    def __init__(self, env, group, width: int) -> None:
        width = _check_width(width)
        if env._amode != 1 or env._omode != 1:
            raise ValueError("the lookahead covers the katago observation and the spatial action mode only")
        index = lambda d: torch.cuda.current_device() if d.index is None else d.index  # noqa: E731
        if getattr(group, "_tables", None) is None or group.device.type != "cuda" or index(group.device) != index(env.device):
            raise ValueError(f"the lookahead runs on a GPU group on the env's device ({env.device}); this group is on {group.device}")
        if env._state.shape[1] != 128:
            raise ValueError(f"the lookahead copies state rows of 128 bytes, the env's have {env._state.shape[1]}")
        self.env, self.group, self.width = env, group, width
        n, dev, hist = env.num_envs, env.device, env._keys.shape[1]
        self.words = _lib.query("ka_lookahead_words", 0, width)
        assert self.words == lookahead_words(width)
        M = n * width
        with torch.cuda.device(dev):
            z = lambda *shape, dtype: torch.zeros(*shape, dtype=dtype, device=dev)  # noqa: E731
            self._records = z(n, self.words, dtype=torch.int32)
            self.child_state = z(M, 128, dtype=torch.uint8)
            self.child_keys = z(M, hist, dtype=torch.int64)
            self.child_checks = z(M, hist, dtype=torch.uint8)
            self.child_bits_in = z(M, MASK_WORDS, dtype=torch.int32)         # the parents' masks: the child step validates against them
            self.child_actions = z(M, dtype=torch.int64)
            self.child_model_of = torch.full((M,), -1, dtype=torch.int32, device=dev)
            self.child_obs = z(M, env._C, 9, 9, dtype=torch.float32)
            self.child_mask_bits = z(M, MASK_WORDS, dtype=torch.int32)
            self.child_rewards = z(M, dtype=torch.float32)
            self.child_terminated = z(M, dtype=torch.bool)
            self.child_truncated = z(M, dtype=torch.bool)
            self.child_players = z(M, dtype=torch.uint8)
            self.child_reason = z(M, dtype=torch.uint8)
            self._terminal_obs = z(M, env._C, 9, 9, dtype=torch.float32)
            self._captured = z(M, dtype=torch.uint8)
            self._ply = z(M, dtype=torch.int16)
            self._material = z(M, dtype=torch.int32)
            self._env_stats = z(4, dtype=torch.int64)
            self._child_err = z(2, dtype=torch.int64)
            self._ws = group._tables.workspace(M)
            self.child_value_logits = self._ws["value"]
            self._counters = z(_lib.query("ka_lookahead_words", 2, width) + 1, dtype=torch.int32)     # stats, then the error word
            self._counters_host = torch.zeros(self._counters.shape, dtype=torch.int32).pin_memory()
        self._nstats = self._counters.shape[0] - 1

    def clear(self) -> None:
        """Zero the counters, the error word and the child step's refusal latch (a round's start)."""
        self._counters.zero_()
        self._child_err.zero_()

    def fork(self, logits, mask_bits, actions, model_of, table, stream) -> None:
        env, K = self.env, int(table.shape[0])
        _lib.call("ka_lookahead_fork", logits, int(logits.dtype == torch.bfloat16), mask_bits, MASK_WORDS, actions, model_of, K,
                  table, env._state, env._keys, env._checks, env._max_ply, self.width, self._records, self.child_state,
                  self.child_keys, self.child_checks, self.child_bits_in, self.child_actions, self.child_model_of,
                  env.num_envs, ACTION_SPACE, stream)

    def step_children(self, stream) -> None:
        env = self.env
        _lib.call("ka_shogi_env_step", self.child_state, self.child_keys, self.child_checks, self.child_actions,
                  env.num_envs * self.width, env._max_ply, env._omode, env._amode, None, self.child_bits_in, self._child_err,
                  self.child_obs, None, self.child_mask_bits, self.child_rewards, self.child_terminated, self.child_truncated,
                  self._terminal_obs, self.child_players, self._captured, self.child_reason, self._ply, self._material,
                  self._env_stats, stream)

    def evaluate(self) -> None:
        self.group._tables.forward(self.child_obs, self.child_model_of, ws=self._ws)

    def choose(self, actions, model_of, table, stream) -> None:
        _lib.call("ka_lookahead_choose", self._records, self.width, table, model_of, int(table.shape[0]),
                  self.child_value_logits, self.child_rewards, self.child_terminated, self.child_truncated, self._child_err,
                  actions, self._counters, self._counters.data_ptr() + 4 * self._nstats, self.env.num_envs, stream)

    def step(self, logits, mask_bits, actions, model_of, table, stream) -> None:
        """The four stages on the current stream (``stream``: its pointer), after the sampler and before ``env.step``:
        ``actions`` (envs,) int64 is overwritten for the active envs.  ``logits`` (envs, 9, 9, 139) or (envs, 11259) fp32 or
        bf16, ``mask_bits`` the env's current packed masks, ``model_of`` (envs,) int32, ``table`` the (K, 4) int32 controls
        table on the device."""
        self.fork(logits, mask_bits, actions, model_of, table, stream)
        self.step_children(stream)
        self.evaluate()
        self.choose(actions, model_of, table, stream)

    def read(self) -> LookaheadStats:
        """At a sync point: the counters since ``clear()`` (one small device -> host copy).  Raises on the error word."""
        self._counters_host.copy_(self._counters)
        c = self._counters_host.numpy()
        err = int(c[self._nstats])
        if err & ERR_CHILD_STEP:
            raise RuntimeError("the lookahead's child step refused an action (word "
                               f"{int(self._child_err[1].item()) or int(self._child_err[0].item()):#x}): a forked row does "
                               "not match the mask it was forked with")
        if err & ERR_VALUE:
            raise RuntimeError("non-finite value logits in the lookahead (a model has diverged)")
        return LookaheadStats(int(c[0]), int(c[1]), int(c[2]))

    def records(self) -> torch.Tensor:
        """The per-env records of the last ``step`` (a copy on the device)."""
        return self._records.clone()
