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

Reply search (``reply_width``, word 3 of the table row, 0..8; 0 = one ply, exactly the above).  With ``reply_width_m = r > 0``
a child ``j`` that is live (neither terminated nor truncated) gets *replies*: its first ``r`` legal actions by the raw policy
logit of model ``m`` on the child's observation -- the logits the children's forward wrote anyway -- in the candidate order;
their softmax priors are recorded and not used, and ``skip_plies`` plays no part.  *Grandchild* ``(j, k)`` is the child's
position after reply ``k``, stepped by ``ka_shogi_env_step`` with the child's full history behind it.  Its value for the root
mover ``v_jk`` is ``0 - reward`` of that step where the game ended there (the env's reward is for the reply's mover), else
``P(W) - P(L)`` of ``softmax(value_logits)`` of model ``m`` on the grandchild's observation (seen by its side to move, who is
the root mover again); a non-finite value logit of a live grandchild makes it -inf and is an error.  ``q_j = min_k v_jk``, the
first minimum; a done child keeps its reward and a live child without a reply candidate keeps its one-ply ``q``.  The choice
is the first maximum of ``u_j = q_j + prior_weight * p_j`` as before; the *one-ply choice* is the same arg-max over the
one-ply ``q``, and a row whose choice differs from it is counted (``LookaheadStats.reply_changed``, flag bit 3).  The one-ply
``q`` of every candidate is still computed, so a non-finite value logit of a live child stays an error.  Seven stages:
fork, step, forward, ``ka_lookahead_fork_replies``, step, forward, ``ka_lookahead_choose_replies``.
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

from ._forked_rows import ForkedRows, PlyStage, check_int, check_search_env, check_weight, controls_rows, table_of

__all__ = ["LookaheadControls", "LookaheadStats", "LookaheadChoice", "LookaheadReplyChoice", "Lookahead", "lookahead_table",
           "lookahead_active", "lookahead_reply_widths", "lookahead_candidates", "lookahead_choose", "lookahead_choose_replies",
           "lookahead_words", "arena_lookahead", "arena_reply_width", "MAX_WIDTH", "MAX_SKIP_PLIES"]

MAX_WIDTH = 8
MAX_SKIP_PLIES = 65535
# record words (csrc/lookahead.hip; ka_lookahead_words reports the sizes)
REC_FLAGS, REC_SLOT, REC_NCAND, REC_ACTION, REC_CAND = 0, 1, 2, 3, 4
FLAG_ACTIVE, FLAG_CHANGED, FLAG_WON, FLAG_REPLY_CHANGED = 1, 2, 4, 8
ERR_VALUE, ERR_CHILD_STEP, ERR_GRANDCHILD_STEP = 1, 2, 4


def lookahead_words(width: int) -> int:
    """32-bit words of one record."""
    return REC_CAND + 3 * int(width)


@dataclass(frozen=True)
class LookaheadControls:
    """One model's lookahead controls.  ``width`` 0 is off; ``reply_width`` 0 searches one ply."""
    width: int = 0
    prior_weight: float = 0.0
    skip_plies: int = 0
    reply_width: int = 0

    OFF: ClassVar["LookaheadControls"]

    def __post_init__(self) -> None:
        for name, hi in (("width", MAX_WIDTH), ("skip_plies", MAX_SKIP_PLIES), ("reply_width", MAX_WIDTH)):
            object.__setattr__(self, name, check_int(name, getattr(self, name), 0, hi))
        object.__setattr__(self, "prior_weight", check_weight("prior_weight", self.prior_weight))
        if self.reply_width > 0 and self.width == 0:
            raise ValueError(f"reply_width {self.reply_width} needs a width above 0: there is no child to reply to")

    def row(self) -> np.ndarray:
        """The table row: int32 width, fp32 prior_weight, int32 skip_plies, int32 reply_width, as four int32."""
        return np.frombuffer(struct.pack("<ifii", self.width, self.prior_weight, self.skip_plies, self.reply_width),
                             dtype=np.int32).copy()


LookaheadControls.OFF = LookaheadControls()


@dataclass
class LookaheadStats:
    """The counters ``ka_lookahead_choose`` / ``ka_lookahead_choose_replies`` add to."""
    searched: int = 0      # positions searched (active envs, summed over the plies)
    changed: int = 0       # choices that differ from the sampler's action
    won: int = 0           # chosen moves that ended the game as a win for the mover
    reply_changed: int = 0  # choices of the reply search that differ from the one-ply choice


def _rows(controls, K: int):
    return controls_rows(controls, K, LookaheadControls, "lookahead")


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


def arena_reply_width(lookahead, num_models: int) -> int:
    """The largest ``reply_width`` of ``MatchArena``'s ``lookahead=`` (0 for None): the grandchild rows are sized by it."""
    return 0 if lookahead is None else max(r.reply_width for r in _rows(lookahead, num_models))


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
    table = table_of(controls, num_models, lookahead_table, "lookahead")
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


def lookahead_reply_widths(controls, model_of, *, num_models: Optional[int] = None, reply_width: int = MAX_WIDTH) -> np.ndarray:
    """Per row: the reply width as the kernels read it from the table -- 0 for a row whose model lies outside ``[0, K)`` or
    whose table row is off or invalid, word 3 outside [0, 8] reads as 0; a value above ``reply_width`` (the launch's) is cut
    to it.  ``skip_plies`` plays no part at this level."""
    table = table_of(controls, num_models, lookahead_table, "lookahead")
    mo = np.asarray(torch.as_tensor(model_of).cpu().numpy(), np.int64).reshape(-1)
    out = np.zeros(mo.shape[0], np.int64)
    for b, m in enumerate(mo):
        if 0 <= m < table.shape[0] and _row_controls(table[m])[0] > 0:
            r = int(table[m, 3])
            out[b] = min(r, int(reply_width)) if 0 <= r <= MAX_WIDTH else 0
    return out


# ---------------------------------------------------------------------------------------------- candidates
def _check_width(width, name: str = "width", lo: int = 1) -> int:
    return check_int(name, width, lo, MAX_WIDTH)


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


# ---------------------------------------------------------------------------------------------- the backed-up choice
@dataclass
class LookaheadReplyChoice:
    slot: torch.Tensor          # (B,)  int32: the chosen slot; -1 for a row without a candidate
    q: torch.Tensor             # (B, width): the backed-up values for the mover (0 in the unused slots)
    u: torch.Tensor             # (B, width): q + prior_weight * prior (-inf in the unused slots); host path fp64, device fp32
    v: torch.Tensor             # (B, width, reply_width): the grandchildren's values for the mover (0 in the unused slots)
    reply_slot: torch.Tensor    # (B, width) int32: the first minimum of v; -1 where q is not a backed-up value
    one_ply_slot: torch.Tensor  # (B,)  int32: the choice of the one-ply search on the same rows
    reply_changed: torch.Tensor  # (B,) bool: the choice differs from the one-ply choice (device path: flag bit 3 of the record)
    error: int                  # bit 0: a non-finite value logit of a live child or grandchild


def lookahead_choose_replies(priors: torch.Tensor, n_cand: torch.Tensor, child_value_logits: torch.Tensor,
                             child_rewards: torch.Tensor, child_done: torch.Tensor, n_reply: torch.Tensor,
                             grand_value_logits: torch.Tensor, grand_rewards: torch.Tensor, grand_done: torch.Tensor,
                             prior_weight) -> LookaheadReplyChoice:
    """The backed-up choice of B rows.  The first five arguments and ``prior_weight`` as for ``lookahead_choose``;
    ``n_reply`` (B, width) the replies of every child (0 = none: the child keeps its one-ply ``q``; a done child's are not
    looked at), ``grand_value_logits`` (B, width, reply_width, 3), ``grand_rewards`` (B, width, reply_width) the env's
    rewards for the reply's mover, ``grand_done`` (B, width, reply_width).  CUDA tensors go through
    ``ka_lookahead_choose_replies``; CPU tensors through the float64 restatement."""
    if priors.dim() != 2 or not 1 <= priors.shape[1] <= MAX_WIDTH or priors.shape[0] < 1:
        raise ValueError(f"priors must have shape (B, width) with B >= 1 and width in [1, {MAX_WIDTH}], got {tuple(priors.shape)}")
    B, width = (int(s) for s in priors.shape)
    if grand_rewards.dim() != 3 or not 1 <= grand_rewards.shape[2] <= MAX_WIDTH:
        raise ValueError(f"grand_rewards must have shape (B, width, reply_width) with reply_width in [1, {MAX_WIDTH}], "
                         f"got {tuple(grand_rewards.shape)}")
    R = int(grand_rewards.shape[2])
    if n_cand.numel() != B or tuple(child_value_logits.shape) != (B, width, 3) or tuple(child_rewards.shape) != (B, width) \
            or tuple(child_done.shape) != (B, width) or tuple(n_reply.shape) != (B, width) \
            or tuple(grand_value_logits.shape) != (B, width, R, 3) or tuple(grand_rewards.shape) != (B, width, R) \
            or tuple(grand_done.shape) != (B, width, R):
        raise ValueError(f"expected n_cand ({B},), child_value_logits ({B}, {width}, 3), child_rewards, child_done and n_reply "
                         f"({B}, {width}), grand_value_logits ({B}, {width}, {R}, 3), grand_rewards and grand_done "
                         f"({B}, {width}, {R})")
    pw = prior_weight.detach().cpu().numpy() if isinstance(prior_weight, torch.Tensor) else prior_weight
    pw = np.broadcast_to(np.asarray(pw, np.float64).reshape(-1), (B,)).copy()
    if not (np.isfinite(pw).all() and (pw >= 0).all()):
        raise ValueError("prior_weight must be finite and >= 0")
    args = (priors, n_cand, child_value_logits, child_rewards, child_done, n_reply, grand_value_logits, grand_rewards,
            grand_done, pw, B, width, R)
    return _choose_replies_device(*args) if priors.is_cuda else _choose_replies_host(*args)


def _loss_minus_win(vl: np.ndarray) -> float:
    e = np.exp(vl - vl.max())
    return (e[2] - e[0]) / e.sum()


def _choose_replies_host(priors, n_cand, vlogits, rewards, done, n_reply, gvl, grw, gdn, pw, B, width, R) -> LookaheadReplyChoice:
    """The semantics of ``ka_lookahead_choose_replies`` in float64."""
    p = priors.double().numpy()
    nc = np.clip(n_cand.reshape(B).numpy().astype(np.int64), 0, width)
    nr = np.clip(n_reply.numpy().astype(np.int64), 0, R)
    vl, rw, dn = vlogits.double().numpy(), rewards.double().numpy(), done.numpy().astype(bool)
    gv, gr, gd = gvl.double().numpy(), grw.double().numpy(), gdn.numpy().astype(bool)
    slot, slot1 = np.full(B, -1, np.int32), np.full(B, -1, np.int32)
    q = np.zeros((B, width), np.float64)
    u = np.full((B, width), -np.inf, np.float64)
    v = np.zeros((B, width, R), np.float64)
    rslot = np.full((B, width), -1, np.int32)
    error = 0
    for b in range(B):
        u1 = np.full(width, -np.inf)
        for j in range(int(nc[b])):
            if dn[b, j]:
                q1 = rw[b, j]
            elif not np.isfinite(vl[b, j]).all():
                q1 = -np.inf
                error |= ERR_VALUE
            else:
                q1 = _loss_minus_win(vl[b, j])                       # the child is seen by its side to move
            q[b, j] = q1
            if not dn[b, j] and nr[b, j] > 0:                        # a live child with replies: the worst of them for the mover
                for k in range(int(nr[b, j])):
                    if gd[b, j, k]:
                        v[b, j, k] = 0.0 - gr[b, j, k]               # the env's reward is for the reply's mover
                    elif not np.isfinite(gv[b, j, k]).all():
                        v[b, j, k] = -np.inf
                        error |= ERR_VALUE
                    else:
                        v[b, j, k] = 0.0 - _loss_minus_win(gv[b, j, k])   # seen by the root mover again: P(W) - P(L)
                    if k == 0 or v[b, j, k] < v[b, j, rslot[b, j]]:  # ties keep the lower slot
                        rslot[b, j] = k
                q[b, j] = v[b, j, rslot[b, j]]
            u1[j] = q1 + pw[b] * p[b, j] if pw[b] > 0 else q1
            u[b, j] = q[b, j] + pw[b] * p[b, j] if pw[b] > 0 else q[b, j]
            if j == 0 or u1[j] > u1[slot1[b]]:
                slot1[b] = j
            if j == 0 or u[b, j] > u[b, slot[b]]:                    # ties keep the lower slot
                slot[b] = j
    return LookaheadReplyChoice(torch.from_numpy(slot), torch.from_numpy(q), torch.from_numpy(u), torch.from_numpy(v),
                                torch.from_numpy(rslot), torch.from_numpy(slot1), torch.from_numpy(slot != slot1), error)


def _choose_replies_device(priors, n_cand, vlogits, rewards, done, n_reply, gvl, grw, gdn, pw, B, width, R) -> LookaheadReplyChoice:
    dev = priors.device
    with torch.cuda.device(dev):
        W, RW = lookahead_words(width), lookahead_words(R)
        f32 = lambda t: t.to(device=dev, dtype=torch.float32).contiguous()  # noqa: E731
        u8 = lambda t: t.to(device=dev, dtype=torch.uint8).contiguous()  # noqa: E731
        rec = torch.zeros(B, W, dtype=torch.int32, device=dev)
        nc = n_cand.reshape(B).to(device=dev, dtype=torch.int32).clamp(0, width)
        rec[:, REC_FLAGS] = (nc > 0).int()
        rec[:, REC_NCAND] = nc
        rec[:, REC_CAND:REC_CAND + width] = torch.arange(width, dtype=torch.int32, device=dev)      # candidate j = "action" j
        rec.view(torch.float32)[:, REC_CAND + width:REC_CAND + 2 * width] = f32(priors)
        rrec = torch.zeros(B * width, RW, dtype=torch.int32, device=dev)
        nr = n_reply.reshape(B * width).to(device=dev, dtype=torch.int32).clamp(0, R)
        rrec[:, REC_FLAGS] = (nr > 0).int()
        rrec[:, REC_NCAND] = nr
        rrec[:, REC_CAND:REC_CAND + R] = torch.arange(R, dtype=torch.int32, device=dev)
        table = torch.zeros(B, 4, dtype=torch.int32, device=dev)            # one table row per row of the batch
        table[:, 0], table[:, 3] = width, R
        table.view(torch.float32)[:, 1] = torch.from_numpy(pw.astype(np.float32)).to(dev)
        actions = torch.full((B,), -1, dtype=torch.int64, device=dev)
        stats = torch.zeros(_lib.query("ka_lookahead_words", 2, width), dtype=torch.int32, device=dev)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        dn, gd = u8(done), u8(gdn)
        _lib.call("ka_lookahead_choose_replies", rec, width, rrec, R, table, torch.arange(B, dtype=torch.int32, device=dev), B,
                  f32(vlogits), f32(rewards), dn, torch.zeros_like(dn), None, f32(gvl), f32(grw), gd, torch.zeros_like(gd), None,
                  actions, stats, err, B, _lib.stream_ptr(dev))
        q = rec.view(torch.float32)[:, REC_CAND + 2 * width:REC_CAND + 3 * width]
        used = torch.arange(width, device=dev)[None, :] < nc[:, None]
        w32 = table.view(torch.float32)[:, 1:2]
        u = torch.where(used, torch.where(w32 > 0, q + w32 * f32(priors), q), torch.full_like(q, float("-inf")))
        slot = torch.where(nc > 0, rec[:, REC_SLOT], torch.full_like(nc, -1))
        backed = used & ~dn.bool() & (nr.reshape(B, width) > 0)
        rslot = torch.where(backed, rrec[:, REC_SLOT].reshape(B, width), torch.full_like(nr.reshape(B, width), -1))
        v = rrec.view(torch.float32)[:, REC_CAND + 2 * R:REC_CAND + 3 * R].reshape(B, width, R)
        # the one-ply choice is not recorded as a slot: flag bit 3 says whether it differs, and the caller has ka_lookahead_choose
        one = lookahead_choose(priors, n_cand, vlogits, rewards, done, pw).slot
        return LookaheadReplyChoice(slot, q, u, v, rslot, one, (rec[:, REC_FLAGS] & FLAG_REPLY_CHANGED) != 0, int(err.item()))


# ---------------------------------------------------------------------------------------------- in the ply
class Lookahead:
    """The child rows of a device ``VecEnv``, the second forward workspace and the stages of the lookahead.  Everything is
    allocated here, once: ``width`` child rows per env, each a state row, a key / check history row, two packed mask rows,
    the step's outputs and a row of the group's workspace; with ``reply_width > 0`` also ``width * reply_width`` grandchild
    rows per env of the same kind, a third workspace and a reply record per child.  ``records()`` (envs, 4 + 3 width) int32
    are the envs' records of the last ``step``, ``reply_records()`` (envs * width, 4 + 3 reply_width) the children's."""

    def __init__(self, env, group, width: int, reply_width: int = 0) -> None:
        width = _check_width(width)
        reply_width = _check_width(reply_width, "reply_width", 0)
        check_search_env(env, group, "the lookahead")
        self.env, self.group, self.width, self.reply_width = env, group, width, reply_width
        n, dev = env.num_envs, env.device
        self.words = _lib.query("ka_lookahead_words", 0, width)
        assert self.words == lookahead_words(width)
        assert max(width, reply_width) <= _lib.query("ka_lookahead_words", 3, 0) == _lib.query("ka_lookahead_words", 4, 0) == MAX_WIDTH
        M = n * width
        with torch.cuda.device(dev):
            z = lambda *shape, dtype: torch.zeros(*shape, dtype=dtype, device=dev)  # noqa: E731
            self._records = z(n, self.words, dtype=torch.int32)
            self._child = c = ForkedRows(env, width, group)
            c.alias(self, "child")                         # child_state .. child_reason, child_model_of, child_logits, _child_err
            self._ws = c.ws
            self._grand: Optional[ForkedRows] = None
            if reply_width:
                self.reply_words = _lib.query("ka_lookahead_words", 0, reply_width)
                self._reply_records = z(M, self.reply_words, dtype=torch.int32)
                self._grand = ForkedRows(c, reply_width, group)
                self._grand.alias(self, "grand")
            self._counters = z(_lib.query("ka_lookahead_words", 2, width) + 1, dtype=torch.int32)     # stats, then the error word
            self._counters_host = torch.zeros(self._counters.shape, dtype=torch.int32).pin_memory()
        self._nstats = self._counters.shape[0] - 1

    def clear(self) -> None:
        """Zero the counters, the error word and the refusal latches of the child and grandchild steps (a round's start)."""
        self._counters.zero_()
        self._child_err.zero_()
        if self._grand is not None:
            self._grand_err.zero_()

    def fork(self, logits, mask_bits, actions, model_of, table, stream) -> None:
        env, K = self.env, int(table.shape[0])
        _lib.call("ka_lookahead_fork", logits, int(logits.dtype == torch.bfloat16), mask_bits, MASK_WORDS, actions, model_of, K,
                  table, env._state, env._keys, env._checks, env._max_ply, self.width, self._records, self.child_state,
                  self.child_keys, self.child_checks, self.child_bits_in, self.child_actions, self.child_model_of,
                  env.num_envs, ACTION_SPACE, stream)

    def step_children(self, stream) -> None:
        self._child.step(stream)

    def evaluate(self) -> None:
        self.group._tables.forward(self.child_obs, self.child_model_of, ws=self._ws)

    def choose(self, actions, model_of, table, stream) -> None:
        _lib.call("ka_lookahead_choose", self._records, self.width, table, model_of, int(table.shape[0]),
                  self.child_value_logits, self.child_rewards, self.child_terminated, self.child_truncated, self._child_err,
                  actions, self._counters, self._counters.data_ptr() + 4 * self._nstats, self.env.num_envs, stream)

    def _need_replies(self) -> ForkedRows:
        if self._grand is None:
            raise ValueError("this Lookahead was built with reply_width=0: it holds no grandchild rows")
        return self._grand

    def fork_replies(self, table, stream) -> None:
        """After ``evaluate``: the replies of every live child from the child logits in the workspace, and the grandchild rows."""
        g, c, env = self._need_replies(), self._child, self.env
        _lib.call("ka_lookahead_fork_replies", self.child_logits, 0, c.mask_bits, MASK_WORDS, c.model_of, int(table.shape[0]),
                  table, c.state, c.keys, c.checks, c.terminated, c.truncated, env._max_ply, self.reply_width,
                  self._reply_records, g.state, g.keys, g.checks, g.bits_in, g.actions, g.model_of, c.M, ACTION_SPACE, stream)

    def step_grandchildren(self, stream) -> None:
        self._need_replies().step(stream)

    def evaluate_grandchildren(self) -> None:
        g = self._need_replies()
        self.group._tables.forward(g.obs, g.model_of, ws=g.ws)

    def choose_replies(self, actions, model_of, table, stream) -> None:
        g, c = self._need_replies(), self._child
        _lib.call("ka_lookahead_choose_replies", self._records, self.width, self._reply_records, self.reply_width, table,
                  model_of, int(table.shape[0]), self.child_value_logits, c.rewards, c.terminated, c.truncated, c.err,
                  self.grand_value_logits, g.rewards, g.terminated, g.truncated, g.err, actions, self._counters,
                  self._counters.data_ptr() + 4 * self._nstats, self.env.num_envs, stream)

    def step(self, logits, mask_bits, actions, model_of, table, stream) -> None:
        """The four stages (seven with ``reply_width > 0``) on the current stream (``stream``: its pointer), after the
        sampler and before ``env.step``: ``actions`` (envs,) int64 is overwritten for the active envs.  ``logits``
        (envs, 9, 9, 139) or (envs, 11259) fp32 or bf16, ``mask_bits`` the env's current packed masks, ``model_of`` (envs,)
        int32, ``table`` the (K, 4) int32 controls table on the device."""
        self.fork(logits, mask_bits, actions, model_of, table, stream)
        self.step_children(stream)
        self.evaluate()
        if self._grand is None:
            self.choose(actions, model_of, table, stream)
            return
        self.fork_replies(table, stream)
        self.step_grandchildren(stream)
        self.evaluate_grandchildren()
        self.choose_replies(actions, model_of, table, stream)

    def read(self) -> LookaheadStats:
        """At a sync point: the counters since ``clear()`` (one small device -> host copy).  Raises on the error word."""
        self._counters_host.copy_(self._counters)
        c = self._counters_host.numpy()
        err = int(c[self._nstats])
        for bit, name, words in ((ERR_CHILD_STEP, "child", self._child_err),
                                 (ERR_GRANDCHILD_STEP, "grandchild", None if self._grand is None else self._grand_err)):
            if err & bit:
                raise RuntimeError(f"the lookahead's {name} step refused an action (word "
                                   f"{int(words[1].item()) or int(words[0].item()):#x}): a forked row does "
                                   "not match the mask it was forked with")
        if err & ERR_VALUE:
            raise RuntimeError("non-finite value logits in the lookahead (a model has diverged)")
        return LookaheadStats(int(c[0]), int(c[1]), int(c[2]), int(c[3]))

    def records(self) -> torch.Tensor:
        """The per-env records of the last ``step`` (a copy on the device)."""
        return self._records.clone()

    def reply_records(self) -> torch.Tensor:
        """The per-child reply records of the last ``step`` (a copy on the device): the layout of the env record with
        ``reply_width`` in the place of ``width``; slot and action are the first worst reply for the mover, the ``q`` words
        the grandchildren's values."""
        self._need_replies()
        return self._reply_records.clone()


class LookaheadStage(PlyStage):
    """The lookahead as a loop builds it into its ply (``lookahead=``: a ``LookaheadControls`` for every model, or one per
    model), between the sampler and the mate check: the insight, the game log and the spectator notes describe the move
    actually played.  The child rows and a second forward workspace are sized by the largest ``width`` given, the grandchild
    rows and a third workspace by the largest ``reply_width``; ``set_lookahead`` goes up to them.  With every ``reply_width``
    0 the launches are those of the one-ply lookahead.  ``RoundStats.lookahead`` carries the counters."""

    name, shares_place, STATS = "lookahead", True, LookaheadStats
    _ROWS = "child and grandchild rows"

    @classmethod
    def parse(cls, lookahead, num_models: int, collect: bool) -> Optional["LookaheadStage"]:
        table, width = arena_lookahead(lookahead, num_models, collect)
        return None if table is None else cls(table, width=width, reply_width=arena_reply_width(lookahead, num_models))

    @classmethod
    def _off(cls, num_models: int) -> "LookaheadStage":
        return cls(lookahead_table(None, num_models), width=0, reply_width=0)

    def _engine(self, env, group) -> Optional[Lookahead]:
        return Lookahead(env, group, **self.sizes) if self.sizes["width"] else None

    def _launch(self, logits, mask_bits, actions, model_of, seed, stream) -> None:
        self.engine.step(logits, mask_bits, actions, model_of, self.table, stream)

    def _record(self) -> dict:
        la, w, r = self.engine, self.engine.width, self.engine.reply_width
        cpu = lambda t, *shape: t.cpu().reshape(-1, *shape)  # noqa: E731
        rec = dict(lookahead_records=la.records().cpu(), child_value_logits=cpu(la.child_value_logits, w, 3),
                   child_rewards=cpu(la.child_rewards, w), child_done=cpu(la.child_terminated | la.child_truncated, w),
                   child_obs=la.child_obs.cpu(), child_mask_bits=la.child_mask_bits.cpu())
        if r:
            rec.update(lookahead_reply_records=la.reply_records().cpu(), grand_value_logits=cpu(la.grand_value_logits, w, r, 3),
                       grand_rewards=cpu(la.grand_rewards, w, r), grand_done=cpu(la.grand_terminated | la.grand_truncated, w, r),
                       child_logits=cpu(la.child_logits, ACTION_SPACE))
        return rec
