"""Policy insight: what the reference's showcase shows next to a board (showcase/runner.py:151-211, showcase/heatmap.py)
-- the softmax over the legal moves at a sampling temperature, the top candidates with their probabilities, the heatmap
of the chosen move's family and the win probability -- plus the entropy of that distribution, the rank of the chosen move
and the number of legal moves.

``policy_insight(logits, legal, actions, value_logits)`` computes them for a batch of rows: CUDA tensors in one launch of
``ka_policy_insight`` (csrc/insight.hip), CPU tensors by the float64 restatement below, which is the documented
semantics.  ``insight_dict(record, heat)`` turns one row into the showcase's dict.  ``InsightRecorder`` is the piece the
device rollouts (``SelfPlayRollout``, ``LeagueRollout``, ``MatchArena`` with ``insight=top_k``) put into their ply: one
launch between the sampler and the env step, into buffers allocated once.

A row's record is ``8 + 2 top_k`` 32-bit words (``ka_policy_insight_words``): flags (bit 0 valid, bit 1 the mover's colour,
bit 2 the chosen action is legal), chosen action, n_legal, chosen_rank, chosen_probability, entropy, win_probability, a
reserved word, the ``top_k`` candidate actions and their probabilities.  Deviations from the reference, all on purpose:
every candidate carries its real USI (the reference writes ``a<index>`` for all but the chosen move), candidates with equal
logits are ordered by lower action index (``np.argsort`` leaves the order of ties to the sort), and ranks and the candidate
order compare raw logits, so they do not depend on rounding.
"""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import List, Optional, Sequence

import numpy as np
import torch

from keisei_amd import _lib
from keisei_amd.shogi_gym import ACTION_SPACE, MASK_WORDS, _SFEN, _amode, _decode_action, _square_hodges

__all__ = ["PolicyInsight", "InsightRecorder", "action_usi", "history_fields", "insight_dict", "insight_words",
           "policy_insight", "HEAT_WORDS", "MAX_TOP_K"]

MAX_TOP_K = 8
HEAT_WORDS = 132                   # the slots of a from-square that are board moves; a drop's family fills the first 81
_SLOTS = 139
# record words (csrc/insight.hip; ka_policy_insight_words reports the same numbers)
REC_FLAGS, REC_ACTION, REC_NLEGAL, REC_RANK, REC_PROB, REC_ENTROPY, REC_WIN, REC_TOP = 0, 1, 2, 3, 4, 5, 6, 8
FLAG_VALID, FLAG_COLOUR, FLAG_LEGAL = 1, 2, 4
CANDIDATE_CUT = 0.001              # runner.py:172


def insight_words(top_k: int) -> int:
    """32-bit words of one record."""
    return REC_TOP + 2 * int(top_k)


@dataclass
class PolicyInsight:
    """One field per output of ``ka_policy_insight`` (include/keisei_amd.h, "policy insight"); B rows."""
    chosen_probability: torch.Tensor     # (B,)  p[action]; 0 where the action is not legal
    entropy: torch.Tensor                # (B,)  nats
    n_legal: torch.Tensor                # (B,)  int32
    chosen_rank: torch.Tensor            # (B,)  int32; -1 where the action is not legal
    win_probability: torch.Tensor        # (B,)  softmax(value_logits)[0]; 0 without value logits
    top_actions: torch.Tensor            # (B, top_k) int32; -1 = unused
    top_probabilities: torch.Tensor      # (B, top_k)
    heat: torch.Tensor                   # (B, 132) fp32
    flags: torch.Tensor                  # (B,)  int32: bit 0 valid, bit 1 mover's colour, bit 2 the action is legal
    records: torch.Tensor                # (B, 8 + 2 top_k) int32: the rows as the kernel writes them (``insight_dict``)
    nan_flag: torch.Tensor               # (1,)  int32: != 0 when a legal logit of a valid row is NaN


def _check(logits, legal, actions, value_logits, players, model_of, temperature, top_k):
    if not isinstance(top_k, int) or isinstance(top_k, bool) or not 1 <= top_k <= MAX_TOP_K:
        raise ValueError(f"top_k must be an integer in [1, {MAX_TOP_K}], got {top_k!r}")
    if not (isinstance(temperature, (int, float)) and math.isfinite(temperature) and temperature > 0):
        raise ValueError(f"temperature must be positive and finite, got {temperature!r}")
    if logits.dim() < 2:
        raise ValueError(f"logits must have shape (B, {ACTION_SPACE}) or (B, 9, 9, {_SLOTS}), got {tuple(logits.shape)}")
    B = logits.shape[0]
    A = logits.numel() // B if B else int(np.prod(logits.shape[1:]))
    if A != ACTION_SPACE:
        raise ValueError(f"policy_insight covers the spatial action space only ({ACTION_SPACE} actions), got {A}")
    if logits.dtype not in (torch.float32, torch.bfloat16, torch.float64):
        raise ValueError(f"logits must be float32 or bfloat16, got {logits.dtype}")
    if legal.dtype == torch.bool and legal.numel() == B * ACTION_SPACE:
        packed = False
    elif legal.dtype == torch.int32 and tuple(legal.shape) == (B, MASK_WORDS):
        packed = True
    else:
        raise ValueError(f"legal must be bool (B, {ACTION_SPACE}) or packed int32 (B, {MASK_WORDS}), "
                         f"got {legal.dtype} {tuple(legal.shape)}")
    if actions.numel() != B:
        raise ValueError(f"expected {B} actions, got {actions.numel()}")
    if value_logits is not None and tuple(value_logits.shape) != (B, 3):
        raise ValueError(f"value_logits must have shape ({B}, 3), got {tuple(value_logits.shape)}")
    for name, t in (("players", players), ("model_of", model_of)):
        if t is not None and t.numel() != B:
            raise ValueError(f"expected {B} {name}, got {t.numel()}")
    return B, packed


def policy_insight(logits: torch.Tensor, legal: torch.Tensor, actions: torch.Tensor,
                   value_logits: Optional[torch.Tensor] = None, *, players: Optional[torch.Tensor] = None,
                   temperature: float = 1.0, top_k: int = 3, model_of: Optional[torch.Tensor] = None,
                   num_models: int = 1) -> PolicyInsight:
    """The insight of B rows.  ``logits`` (B, 11259) or (B, 9, 9, 139), fp32 or bf16; ``legal`` bool rows or packed int32
    rows (B, 352), as ``SEResNetGroup.select_actions`` takes them; ``actions`` (B,) the chosen actions; ``value_logits``
    (B, 3) or None; ``players`` (B,) the movers' colours or None; ``model_of`` / ``num_models`` with the sampler's meaning (a
    row outside [0, num_models) is invalid), None = every row seated.  CUDA tensors go through ``ka_policy_insight``;
    CPU tensors through a float64 restatement."""
    B, packed = _check(logits, legal, actions, value_logits, players, model_of, temperature, top_k)
    if logits.is_cuda:
        return _insight_device(logits, legal, actions, value_logits, players, model_of, int(num_models), float(temperature),
                               top_k, B, packed)
    return _insight_host(logits, legal, actions, value_logits, players, model_of, int(num_models), float(temperature),
                         top_k, B, packed)


def _from_records(records: torch.Tensor, heat: torch.Tensor, nan_flag: torch.Tensor, top_k: int) -> PolicyInsight:
    f = records.view(torch.float32)
    return PolicyInsight(chosen_probability=f[:, REC_PROB], entropy=f[:, REC_ENTROPY], n_legal=records[:, REC_NLEGAL],
                         chosen_rank=records[:, REC_RANK], win_probability=f[:, REC_WIN],
                         top_actions=records[:, REC_TOP:REC_TOP + top_k], top_probabilities=f[:, REC_TOP + top_k:REC_TOP + 2 * top_k],
                         heat=heat, flags=records[:, REC_FLAGS], records=records, nan_flag=nan_flag)


def _insight_device(logits, legal, actions, value_logits, players, model_of, K, temperature, top_k, B, packed):
    dev = logits.device
    with torch.cuda.device(dev):
        st = _lib.stream_ptr(dev)
        lg = logits.reshape(B, ACTION_SPACE)
        if lg.dtype == torch.float64:
            lg = lg.float()
        lg = lg.contiguous()
        if packed:
            bits = legal.to(dev).contiguous()
        else:
            bits = torch.zeros(B, MASK_WORDS, dtype=torch.int32, device=dev)
            if B:
                _lib.call("ka_pack_mask_bits", legal.reshape(B, ACTION_SPACE).to(dev).contiguous(), bits, B, ACTION_SPACE, st)
        W = insight_words(top_k)
        records = torch.zeros(B, W, dtype=torch.int32, device=dev)
        heat = torch.zeros(B, HEAT_WORDS, dtype=torch.float32, device=dev)
        nan_flag = torch.zeros(1, dtype=torch.int32, device=dev)
        if B:
            t = lambda x, dt: None if x is None else x.reshape(-1).to(device=dev, dtype=dt).contiguous()  # noqa: E731
            vl = None if value_logits is None else value_logits.to(device=dev, dtype=torch.float32).contiguous()
            _lib.call("ka_policy_insight", lg, int(lg.dtype == torch.bfloat16), bits, MASK_WORDS, t(actions, torch.int64), vl,
                      t(players, torch.uint8), t(model_of, torch.int32), K, temperature, top_k, records, heat, None, 0, None,
                      nan_flag, B, ACTION_SPACE, st)
    return _from_records(records, heat, nan_flag, top_k)


def _unpack(legal: torch.Tensor, B: int, packed: bool) -> torch.Tensor:
    if not packed:
        return legal.reshape(B, ACTION_SPACE)
    j = torch.arange(ACTION_SPACE)
    return ((legal[:, j // 32] >> (j % 32)) & 1).bool()


def _insight_host(logits, legal, actions, value_logits, players, model_of, K, temperature, top_k, B, packed):
    """The semantics of ``ka_policy_insight`` in float64 (runner.py:151-173, heatmap.py:40-49, inference.py:95)."""
    inf = float("inf")
    x = logits.reshape(B, ACTION_SPACE).double()
    mask = _unpack(legal, B, packed)
    act = actions.reshape(B).long()
    n_legal = mask.sum(dim=1)
    seated = torch.ones(B, dtype=torch.bool) if model_of is None else ((model_of.reshape(B) >= 0) & (model_of.reshape(B) < K))
    valid = seated & (n_legal > 0)
    masked = torch.where(mask, x, torch.full_like(x, -inf))                       # runner.py:151-153, with -inf for -1e9
    nan = torch.isnan(masked)
    mx = torch.where(nan, torch.full_like(x, -inf), masked).max(dim=1, keepdim=True).values
    z = (masked - mx) / temperature                                               # :156-158
    e = torch.where(mask, torch.exp(z), torch.zeros_like(z))
    p = e / e.sum(dim=1, keepdim=True)                                            # :159-163 (the total is at least 1)
    plogp = torch.where(p > 0, p * torch.log(p.clamp_min(1e-300)), torch.zeros_like(p))
    entropy = -plogp.sum(dim=1)
    in_range = (act >= 0) & (act < ACTION_SPACE)
    a_cl = act.clamp(0, ACTION_SPACE - 1)
    rows = torch.arange(B)
    legal_act = in_range & mask[rows, a_cl]
    chosen_p = torch.where(legal_act, p[rows, a_cl], torch.zeros(B, dtype=torch.float64))
    rank = torch.where(legal_act, (masked > masked[rows, a_cl][:, None]).sum(dim=1), torch.full((B,), -1))
    # candidates: raw logit descending, equal logits by lower action (a stable sort); -inf and NaN never
    key = torch.where(nan, torch.full_like(x, -inf), masked)
    order = torch.sort(key, dim=1, descending=True, stable=True).indices[:, :top_k]
    used = key.gather(1, order) > -inf
    top_a = torch.where(used, order, torch.full_like(order, -1))
    top_p = torch.where(used, p.gather(1, order), torch.zeros(B, top_k, dtype=torch.float64))
    win = torch.zeros(B, dtype=torch.float64) if value_logits is None else torch.softmax(value_logits.double(), dim=1)[:, 0]
    heat = torch.zeros(B, HEAT_WORDS, dtype=torch.float64)
    for b in torch.nonzero(legal_act & valid).reshape(-1).tolist():               # heatmap.py:40-49
        frm, slot = divmod(int(act[b]), _SLOTS)
        if slot < HEAT_WORDS:
            heat[b] = p[b, frm * _SLOTS:frm * _SLOTS + HEAT_WORDS]
        else:
            heat[b, :81] = p[b, slot::_SLOTS]
    colour = torch.zeros(B, dtype=torch.int64) if players is None else (players.reshape(B).long() & 1)
    flags = (FLAG_VALID + FLAG_COLOUR * colour + FLAG_LEGAL * legal_act.long()) * valid.long()
    v1, v2 = valid, valid[:, None]
    zero = lambda t, v: torch.where(v, t, torch.zeros_like(t))  # noqa: E731
    chosen_p, entropy, win, rank = zero(chosen_p, v1), zero(entropy, v1), zero(win, v1), zero(rank, v1)
    n_out, top_a, top_p, heat = zero(n_legal, v1), zero(top_a, v2), zero(top_p, v2), zero(heat, v2)
    a_rec = zero(torch.where(in_range, act, torch.where(act < 0, torch.full_like(act, -1), torch.full_like(act, ACTION_SPACE))), v1)
    W = insight_words(top_k)
    records = torch.zeros(B, W, dtype=torch.int32)
    fv = records.view(torch.float32)
    records[:, REC_FLAGS], records[:, REC_ACTION] = flags.int(), a_rec.int()
    records[:, REC_NLEGAL], records[:, REC_RANK] = n_out.int(), rank.int()
    fv[:, REC_PROB], fv[:, REC_ENTROPY], fv[:, REC_WIN] = chosen_p.float(), entropy.float(), win.float()
    records[:, REC_TOP:REC_TOP + top_k] = top_a.int()
    fv[:, REC_TOP + top_k:REC_TOP + 2 * top_k] = top_p.float()
    nan_flag = (nan & valid[:, None]).any().int().reshape(1)
    return PolicyInsight(chosen_probability=chosen_p, entropy=entropy, n_legal=n_out.int(), chosen_rank=rank.int(),
                         win_probability=win, top_actions=top_a.int(), top_probabilities=top_p, heat=heat.float(),
                         flags=flags.int(), records=records, nan_flag=nan_flag)


# ---------------------------------------------------------------------------------------------- records -> dicts
def action_usi(action: int, colour: int, action_mode="spatial") -> str:
    """The USI of an action index played by ``colour`` (0 black, 1 white): "7g7f", "8h2b+", "P*5e"; "?" for an index that
    names no move.  The same decode as the spectator feed's ``move_usi``."""
    mv = _decode_action(int(action), int(colour) & 1, _amode(action_mode))
    if mv is None:
        return "?"
    frm, to, promote, drop = mv
    if drop >= 0:
        return f"{_SFEN[drop + 1]}*{_square_hodges(to)}"
    return _square_hodges(frm) + _square_hodges(to) + ("+" if promote else "")


def _record_words(record) -> np.ndarray:
    if isinstance(record, torch.Tensor):
        record = record.detach().cpu().numpy()
    rec = np.ascontiguousarray(record).reshape(-1)
    if rec.dtype.itemsize != 4:
        raise ValueError(f"a record is a row of 32-bit words, got dtype {rec.dtype}")
    rec = rec.view(np.int32)
    if rec.size < insight_words(1) or rec.size > insight_words(MAX_TOP_K) or (rec.size - REC_TOP) % 2:
        raise ValueError(f"a record holds 8 + 2 top_k words with top_k in [1, {MAX_TOP_K}], got {rec.size}")
    return rec


def _candidates(rec: np.ndarray, colour: int, action_mode) -> list:
    """runner.py:169-173, :193-194 -- with the real USI of every candidate."""
    k = (rec.size - REC_TOP) // 2
    probs = rec[REC_TOP + k:REC_TOP + 2 * k].view(np.float32)
    out = []
    for a, p in zip(rec[REC_TOP:REC_TOP + k].tolist(), probs.tolist()):
        if a >= 0 and p > CANDIDATE_CUT:
            out.append({"action": int(a), "probability": round(float(p), 4), "usi": action_usi(a, colour, action_mode)})
    return out


def history_fields(record, action_mode="spatial") -> dict:
    """What a ``move_history`` entry gains from the move's record: ``probability``, ``rank``, ``entropy``,
    ``win_probability`` and ``top_candidates`` (None / [] for an invalid record: an unseated row)."""
    rec = _record_words(record)
    flags = int(rec[REC_FLAGS])
    if not flags & FLAG_VALID:
        return {"probability": None, "rank": None, "entropy": None, "win_probability": None, "top_candidates": []}
    f = rec.view(np.float32)
    return {"probability": float(f[REC_PROB]), "rank": int(rec[REC_RANK]), "entropy": float(f[REC_ENTROPY]),
            "win_probability": float(f[REC_WIN]), "top_candidates": _candidates(rec, (flags >> 1) & 1, action_mode)}


def insight_dict(record, heat, action_mode="spatial") -> Optional[dict]:
    """One row as the showcase's figures: ``chosen_probability``, ``chosen_rank``, ``legal_moves``, ``policy_entropy``,
    ``win_probability``, ``top_candidates`` (runner.py:169-173: the entries with p > 0.001, ``probability`` rounded to 4
    places, each with its real ``usi``) and ``move_heatmap`` (``build_heatmap``'s ``{usi: p}`` over the chosen move's family,
    finite p > 0), plus ``action`` and ``move_usi`` of the chosen move.  None for an invalid record."""
    if _amode(action_mode) != 1:
        raise ValueError("policy insight covers the spatial action mode only")
    rec = _record_words(record)
    flags = int(rec[REC_FLAGS])
    if not flags & FLAG_VALID:
        return None
    if isinstance(heat, torch.Tensor):
        heat = heat.detach().cpu().numpy()
    heat = np.asarray(heat, dtype=np.float64).reshape(-1)
    if heat.size != HEAT_WORDS:
        raise ValueError(f"a heat row holds {HEAT_WORDS} floats, got {heat.size}")
    f = rec.view(np.float32)
    colour, action = (flags >> 1) & 1, int(rec[REC_ACTION])
    heatmap = {}
    if flags & FLAG_LEGAL:
        frm, slot = divmod(action, _SLOTS)
        family = [frm * _SLOTS + s for s in range(HEAT_WORDS)] if slot < HEAT_WORDS else [sq * _SLOTS + slot for sq in range(81)]
        for a, p in zip(family, heat.tolist()):
            usi = action_usi(a, colour, action_mode)
            if math.isfinite(p) and p > 0.0 and usi != "?":    # heatmap.py:46; a slot that points off the board names no move
                heatmap[usi] = float(p)
    return {"action": action, "move_usi": action_usi(action, colour, action_mode) if flags & FLAG_LEGAL else "",
            "chosen_probability": float(f[REC_PROB]), "chosen_rank": int(rec[REC_RANK]), "legal_moves": int(rec[REC_NLEGAL]),
            "policy_entropy": float(f[REC_ENTROPY]), "win_probability": float(f[REC_WIN]),
            "top_candidates": _candidates(rec, colour, action_mode), "move_heatmap": heatmap}


# ---------------------------------------------------------------------------------------------- in the ply
class InsightRecorder:
    """The insight buffers of a device rollout and its launch.  ``last`` (envs, words) and ``heat`` (envs, 132) hold every
    env's last move; with an env built with ``move_history=True``, ``hist`` (envs, row_len, words) holds a record per move
    of the game in progress, indexed by the env's spectator move count.  Everything is allocated here, once."""

    def __init__(self, env, top_k: int, temperature: float = 1.0) -> None:
        if not isinstance(top_k, int) or isinstance(top_k, bool) or not 1 <= top_k <= MAX_TOP_K:
            raise ValueError(f"insight (the top_k of the policy insight) must be 0 or an integer in [1, {MAX_TOP_K}], got {top_k!r}")
        if not (isinstance(temperature, (int, float)) and math.isfinite(temperature) and temperature > 0):
            raise ValueError(f"insight_temperature must be positive and finite, got {temperature!r}")
        if env._amode != 1:
            raise ValueError("policy insight covers the spatial action mode only")
        self.env, self.top_k, self.temperature = env, int(top_k), float(temperature)
        self.words = _lib.query("ka_policy_insight_words", 0, self.top_k)
        assert self.words == insight_words(self.top_k)
        n, dev = env.num_envs, env.device
        self.last = torch.zeros(n, self.words, dtype=torch.int32, device=dev)
        self.heat = torch.zeros(n, HEAT_WORDS, dtype=torch.float32, device=dev)
        self.hist = None
        if env._hist is not None:
            self.hist = torch.zeros(n, env._hist.shape[1], self.words, dtype=torch.int32, device=dev)

    def clear(self) -> None:
        """After the env's reset: no env has moved yet."""
        self.last.zero_()
        self.heat.zero_()

    def step(self, logits, mask_bits, actions, value_logits, players, model_of, num_models: int, flags, stream) -> None:
        """One ``ka_policy_insight`` launch: after the sampler, before ``env.step`` (the move count is the one before it)."""
        env = self.env
        _lib.call("ka_policy_insight", logits, 0, mask_bits, MASK_WORDS, actions, value_logits, players, model_of,
                  int(num_models), self.temperature, self.top_k, self.last, self.heat, self.hist,
                  0 if self.hist is None else self.hist.shape[1], env._hist_count, flags, env.num_envs, ACTION_SPACE, stream)

    def annotate(self, data: List[dict], envs: Optional[Sequence[int]]) -> List[dict]:
        """``data``: ``get_spectator_data(envs)``.  Every dict gains ``insight`` (one more copy of exactly the rows asked
        for); with a history, every ``move_history`` entry gains ``history_fields`` of its move."""
        env = self.env
        both = torch.cat([self.last, self.heat.view(torch.int32)], dim=1)
        idx = None if envs is None else torch.as_tensor([int(e) for e in envs], dtype=torch.int64, device=env.device)
        if idx is not None:
            both = both[idx]
        both = both.cpu().numpy()
        hist = None
        longest = max((len(d["move_history"]) for d in data), default=0)
        if self.hist is not None and longest:
            rows = self.hist if idx is None else self.hist[idx]
            hist = rows[:, :longest].cpu().numpy()
        mode = "spatial"
        for j, d in enumerate(data):
            d["insight"] = insight_dict(both[j, :self.words], both[j, self.words:].view(np.float32), mode)
            if self.hist is not None:
                for i, entry in enumerate(d["move_history"]):
                    entry.update(history_fields(hist[j, i], mode))
        return data
