"""Sampling controls for the device ply: a temperature, a top-k cut and an opening schedule per model.

The play sampler (``ka_policy_sample_play``) draws at temperature 1 from the full masked softmax, as the reference's
rollout and tournament code does (``Categorical(probs).sample()``).  The reference's showcase plays at
``SAMPLING_TEMPERATURE = 0.5`` (showcase/runner.py:52, :155-163), evaluation wants exploratory opening plies and sharp or
greedy play behind them, and a league wants sharper or more diverse opponents: ``ka_policy_sample_ctl``
(csrc/sampling.hip) is the play sampler with those controls, read per model from a small table in device memory.

``SamplingControls`` is one row of that table, ``controls_table`` builds the table, ``sample_controlled`` draws for a
batch of rows: CUDA tensors in one launch of the kernel, CPU tensors by the float64 restatement below, which is the
documented semantics.  ``MatchArena(sampling=)`` and ``LeagueRollout(opponent_sampling=)`` put the kernel into their ply.

Semantics of a seated row (model ``m = model_of[b]`` in ``[0, K)``, game ply ``p``, controls = row ``m`` of the table):
``T = opening_temperature if p < opening_plies else temperature``; the support ``S`` is every legal action when
``top_k == 0`` or ``n_legal <= top_k``, else the ``top_k`` legal actions that come first by raw logit descending, equal
logits by lower action (the candidate order of the policy insight); ``T == 0`` plays the first action of that order with
probability 1; ``T > 0`` draws from ``q_j ~ exp((z_j - max_S z) / T)`` over ``S`` by inverse CDF in ascending action
order, with the play sampler's uniform of ``(seed, row)``.  ``log_probs`` is ``log(clamp(q, eps, 1 - eps))`` with
``eps = FLT_EPSILON``.  A row outside ``[0, K)`` takes its first legal action with log-prob 0.  The neutral row
(``T == 1``, ``top_k == 0``) is the play sampler, bit for bit.
"""
from __future__ import annotations

import math
import struct
from dataclasses import dataclass
from typing import ClassVar, Optional

import numpy as np
import torch

from keisei_amd import _lib

from ._forked_rows import check_int, table_of

__all__ = ["SamplingControls", "ControlledSample", "controls_table", "sample_controlled", "sample_uniform",
           "arena_controls", "league_controls", "MAX_TOP_K", "MAX_OPENING_PLIES", "GAME_PLY_BYTE"]

MAX_TOP_K = 64
MAX_OPENING_PLIES = 65535
GAME_PLY_BYTE = 100                # the u32 game ply inside an env state row (csrc/shogi_env.hip)
_EPS = 1.1920928955078125e-07      # FLT_EPSILON
_M64 = (1 << 64) - 1


def _temperature(name: str, t) -> float:
    if isinstance(t, bool) or not isinstance(t, (int, float)) or not math.isfinite(t) or t < 0:
        raise ValueError(f"{name} must be finite and >= 0, got {t!r}")
    return float(t)


@dataclass(frozen=True)
class SamplingControls:
    """One model's sampling controls.  ``temperature`` 0 is greedy; ``opening_temperature`` (None = ``temperature``) holds
    for the game plies below ``opening_plies``; ``top_k`` 0 is no cut."""
    temperature: float = 1.0
    opening_temperature: Optional[float] = None
    opening_plies: int = 0
    top_k: int = 0

    GREEDY: ClassVar["SamplingControls"]
    NEUTRAL: ClassVar["SamplingControls"]

    def __post_init__(self) -> None:
        object.__setattr__(self, "temperature", _temperature("temperature", self.temperature))
        if self.opening_temperature is not None:
            object.__setattr__(self, "opening_temperature", _temperature("opening_temperature", self.opening_temperature))
        for name, hi in (("opening_plies", MAX_OPENING_PLIES), ("top_k", MAX_TOP_K)):
            object.__setattr__(self, name, check_int(name, getattr(self, name), 0, hi))

    def row(self) -> np.ndarray:
        """The table row: fp32 temperature, fp32 opening temperature, int32 opening_plies, int32 top_k, as four int32."""
        t_open = self.temperature if self.opening_temperature is None else self.opening_temperature
        return np.frombuffer(struct.pack("<ffii", self.temperature, t_open, self.opening_plies, self.top_k), dtype=np.int32).copy()

    def effective(self, ply: Optional[int]) -> "SamplingControls":
        """The single-temperature controls that hold at game ply ``ply`` (None = past every opening)."""
        if ply is None or ply >= self.opening_plies or self.opening_temperature is None:
            return SamplingControls(self.temperature, None, 0, self.top_k)
        return SamplingControls(self.opening_temperature, None, 0, self.top_k)


SamplingControls.GREEDY = SamplingControls(temperature=0.0)
SamplingControls.NEUTRAL = SamplingControls()


def controls_table(sampling, K: int) -> np.ndarray:
    """The ``(K, 4)`` int32 controls table (floats bit-cast).  ``sampling``: None (K neutral rows), one
    ``SamplingControls`` (every model) or a sequence of exactly K."""
    if isinstance(K, bool) or not isinstance(K, (int, np.integer)) or K < 1:
        raise ValueError(f"a controls table needs at least one row, got K = {K!r}")
    K = int(K)
    if sampling is None:
        rows = [SamplingControls.NEUTRAL] * K
    elif isinstance(sampling, SamplingControls):
        rows = [sampling] * K
    elif isinstance(sampling, (list, tuple)):
        rows = list(sampling)
        if len(rows) != K:
            raise ValueError(f"expected {K} SamplingControls (one per model), got {len(rows)}")
        for r in rows:
            if not isinstance(r, SamplingControls):
                raise ValueError(f"every entry must be a SamplingControls, got {type(r).__name__}")
    else:
        raise ValueError(f"sampling must be None, a SamplingControls or a sequence of {K}, got {type(sampling).__name__}")
    return np.stack([r.row() for r in rows]).astype(np.int32, copy=False)


def arena_controls(sampling, num_models: int, collect: bool) -> Optional[np.ndarray]:
    """``MatchArena``'s reading of ``sampling=``: None stays None (the ply keeps the play sampler), everything else is a
    table of ``num_models`` rows -- refused with ``collect=True``, where ``DynamicTrainer`` treats the recorded actions as
    the entry's own policy, which a tempered draw is not."""
    if sampling is None:
        return None
    if collect:
        raise ValueError("sampling controls cannot be combined with collect=True: DynamicTrainer treats the recorded "
                         "actions as draws from the entry's own policy, and a tempered, cut or greedy draw is not one")
    return controls_table(sampling, num_models)


def league_controls(opponent_sampling, num_opponents: int) -> Optional[np.ndarray]:
    """``LeagueRollout``'s reading of ``opponent_sampling=``: None stays None; otherwise a table of ``1 + num_opponents``
    rows whose row 0, the learner, is always neutral (its draws are the PPO behaviour policy)."""
    if opponent_sampling is None:
        return None
    if isinstance(opponent_sampling, (list, tuple)) and len(opponent_sampling) != num_opponents:
        raise ValueError(f"expected {num_opponents} SamplingControls (one per opponent), got {len(opponent_sampling)}")
    return np.concatenate([controls_table(None, 1), controls_table(opponent_sampling, num_opponents)])


# ---------------------------------------------------------------------------------------------- the uniform
def _mix(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & _M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _M64
    return x ^ (x >> 31)


def sample_uniform(seed: int, row: int) -> float:
    """The sampler's uniform of ``(seed, row)``: the top 24 bits of ``mix(seed ^ mix(row + 0x5851F42D4C957F2D))`` over 2^24,
    with the splitmix64 finaliser as ``mix`` (csrc/common.h, ``ka_mix64``)."""
    h = _mix((int(seed) & _M64) ^ _mix((int(row) + 0x5851F42D4C957F2D) & _M64))
    return (h >> 40) / 16777216.0


# ---------------------------------------------------------------------------------------------- one batch
@dataclass
class ControlledSample:
    actions: torch.Tensor                 # (B,)  int64
    log_probs: torch.Tensor               # (B,)  fp32 on the device, fp64 on the host
    n_legal: torch.Tensor                 # (B,)  int32: every legal action, not |S|
    flags: torch.Tensor                   # (2,)  int32: [0] a NaN logit, [1] a row without a legal action
    probs: Optional[torch.Tensor] = None  # (B, A) fp64, the distribution drawn from: host path only


def sample_controlled(logits: torch.Tensor, legal: torch.Tensor, seed, *, controls, model_of: Optional[torch.Tensor] = None,
                      plies: Optional[torch.Tensor] = None, num_models: Optional[int] = None) -> ControlledSample:
    """One draw per row.  ``logits`` (B, A) or (B, 9, 9, 139), fp32 or bf16; ``legal`` bool rows or packed int32 rows
    (B, ceil(A / 32)); ``seed`` an int (or a one-element int64 tensor); ``controls`` what ``controls_table`` takes, or a
    (K, 4) int32 table; ``model_of`` (B,) each row's model (None = model 0), rows outside ``[0, K)`` are unseated; ``plies``
    (B,) each row's game ply (None = past every opening).  K is ``num_models``, else the length of ``controls``, else 1.
    CUDA tensors go through ``ka_policy_sample_ctl``; CPU tensors through the float64 restatement, which also returns the
    distribution drawn from in ``probs``."""
    if logits.dim() < 2:
        raise ValueError(f"logits must have shape (B, A) or (B, 9, 9, 139), got {tuple(logits.shape)}")
    if logits.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError(f"logits must be float32 or bfloat16, got {logits.dtype}")
    B = int(logits.shape[0])
    if B < 1:
        raise ValueError("sample_controlled needs at least one row")
    A = logits.numel() // B
    words = (A + 31) // 32
    if legal.dtype == torch.bool and legal.numel() == B * A:
        packed = False
    elif legal.dtype == torch.int32 and tuple(legal.shape) == (B, words):
        packed = True
    else:
        raise ValueError(f"legal must be bool (B, {A}) or packed int32 (B, {words}), got {legal.dtype} {tuple(legal.shape)}")
    table = table_of(controls, num_models, controls_table, "controls")
    K = table.shape[0]
    model_of = None if model_of is None else torch.as_tensor(model_of)
    plies = None if plies is None else torch.as_tensor(plies)
    for name, t in (("model_of", model_of), ("plies", plies)):
        if t is not None and t.numel() != B:
            raise ValueError(f"expected {B} {name}, got {t.numel()}")
    if plies is not None:
        plies = torch.as_tensor(plies).reshape(B).to(device="cpu", dtype=torch.int64)
        if bool((plies < 0).any()) or bool((plies > 0xFFFFFFFF).any()):
            raise ValueError("plies are unsigned 32-bit game plies")
    seed = int(seed.item()) if isinstance(seed, torch.Tensor) else int(seed)
    if logits.is_cuda:
        return _sample_device(logits.reshape(B, A), legal, seed, table, model_of, plies, B, A, K, packed)
    return _sample_host(logits.reshape(B, A), legal, seed, table, model_of, plies, B, A, K, packed)


def _sample_device(logits, legal, seed, table, model_of, plies, B, A, K, packed) -> ControlledSample:
    dev = logits.device
    with torch.cuda.device(dev):
        lg = logits.contiguous()
        mask = legal.to(dev).contiguous() if packed else legal.reshape(B, A).to(dev).contiguous()
        ctl = torch.from_numpy(table).to(dev)
        seed_dev = torch.tensor([seed if seed < (1 << 63) else seed - (1 << 64)], dtype=torch.int64, device=dev)
        mo = torch.zeros(B, dtype=torch.int32, device=dev) if model_of is None else \
            model_of.reshape(B).to(device=dev, dtype=torch.int32).contiguous()
        # (an int32 column holds the u32 bit pattern: the kernel reads the word unsigned)
        pl = None if plies is None else \
            torch.from_numpy(plies.numpy().astype(np.uint32).view(np.int32)).to(dev)
        actions = torch.zeros(B, dtype=torch.int64, device=dev)
        logp = torch.zeros(B, dtype=torch.float32, device=dev)
        nlegal = torch.zeros(B, dtype=torch.int32, device=dev)
        flags = torch.zeros(2, dtype=torch.int32, device=dev)
        _lib.call("ka_policy_sample_ctl", lg, int(lg.dtype == torch.bfloat16), mask, (A + 31) // 32 if packed else 0, seed_dev,
                  mo, K, ctl, pl, 4, actions, logp, nlegal, flags, B, A, _lib.stream_ptr(dev))
    return ControlledSample(actions=actions, log_probs=logp, n_legal=nlegal, flags=flags)


def _row_controls(row: np.ndarray):
    """(temperature, opening_temperature, opening_plies, top_k) of a table row as the kernel reads it: a row with top_k
    outside [0, 64] or a negative or non-finite temperature is the neutral row."""
    t_late, t_open = (float(x) for x in row[:2].view(np.float32))
    opening, k = int(row[2]), int(row[3])
    if not (math.isfinite(t_late) and t_late >= 0 and math.isfinite(t_open) and t_open >= 0 and 0 <= k <= MAX_TOP_K):
        return 1.0, 1.0, 0, 0
    return t_late, t_open, opening, k


def _sample_host(logits, legal, seed, table, model_of, plies, B, A, K, packed) -> ControlledSample:
    """The semantics of ``ka_policy_sample_ctl`` in float64."""
    x = logits.double().numpy()
    if packed:
        j = np.arange(A)
        mask = ((legal.numpy().view(np.uint32)[:, j // 32] >> (j % 32).astype(np.uint32)) & 1).astype(bool)
    else:
        mask = legal.reshape(B, A).numpy()
    mo = np.zeros(B, np.int64) if model_of is None else model_of.reshape(B).numpy().astype(np.int64)
    pl = None if plies is None else plies.reshape(B).numpy().astype(np.int64)
    actions, logp = np.zeros(B, np.int64), np.zeros(B, np.float64)
    probs = np.zeros((B, A), np.float64)
    flags = np.zeros(2, np.int32)
    n_legal = mask.sum(axis=1).astype(np.int32)
    if np.isnan(x).any():
        flags[0] = 1
    for b in range(B):
        idx = np.flatnonzero(mask[b])                                  # ascending action order
        if idx.size == 0:
            flags[1] = 1
            continue
        if not 0 <= mo[b] < K:                                         # unseated: the first legal action, log-prob 0
            actions[b] = idx[0]
            continue
        t_late, t_open, opening, k = _row_controls(table[mo[b]])
        T = t_open if (pl is not None and opening > 0 and pl[b] < opening) else t_late
        z = x[b, idx]
        key = np.where(np.isnan(z), -np.inf, z)
        order = np.argsort(-key, kind="stable")                        # logit descending, equal logits by lower action
        if T == 0:
            a = idx[order[0]]
            actions[b], probs[b, a] = a, 1.0
            logp[b] = math.log(1.0 - _EPS)
            continue
        if k > 0 and idx.size > k:
            keep = np.sort(order[:k])
            idx, key = idx[keep], key[keep]
        with np.errstate(over="ignore", invalid="ignore"):                 # (a NaN logit is flagged; here it weighs nothing)
            e = np.where(key == key.max(), 1.0, np.exp((key - key.max()) / T))
        total = e.sum()
        q = e / total
        probs[b, idx] = q
        target = sample_uniform(seed, b) * total
        hit = np.flatnonzero(np.cumsum(e) > target)
        pick = int(hit[0]) if hit.size else int(np.flatnonzero(e > 0)[-1])      # rounding left target >= total: the last of S
        actions[b] = idx[pick]
        logp[b] = math.log(min(max(q[pick], _EPS), 1.0 - _EPS))
    return ControlledSample(actions=torch.from_numpy(actions), log_probs=torch.from_numpy(logp),
                            n_legal=torch.from_numpy(n_legal), flags=torch.from_numpy(flags), probs=torch.from_numpy(probs))
