"""Exploration for the visit-count search (``mcts_search.py``): Dirichlet noise mixed into the root priors and, for the first
plies of a game, the move drawn in proportion to the root visits.

Without them the search is a function of the position: the most visited root candidate is played, ties to the lower slot, so
two models play one game from one start position however many envs they are given, and the visit targets a trainer drains
are thousands of copies of one line.  Both controls live inside the ply -- the priors and the tree exist in device memory for
one ply only -- in ``ka_mcts_root_noise`` (csrc/mcts_explore.hip) and in a branch of the advance
(``ka_mcts_advance_explore``, csrc/mcts.hip).  The float64 restatements below are the meaning.

Controls.  Row ``m`` of the exploration table belongs to model ``m``: fp32 ``noise_fraction`` epsilon in [0, 1], fp32
``noise_alpha`` in [0.01, 100] (not looked at when epsilon is 0), int32 ``sample_plies`` in [0, 65535], one reserved word.  A
row with a word out of range reads as ``OFF``, and so does a model outside ``[0, K)``.

Random numbers.  ``seed`` is the int64 at the head of the loop's state array, the word the sampler reads this ply.  With
``mix`` the splitmix64 finaliser behind every draw of the library (csrc/common.h ``ka_mix64``, ``league_rollout._mix``), the
stream of env ``e`` for purpose ``C`` is ``h = mix(seed ^ mix(e + C))``, draw ``i`` of it ``r_i = mix(h + i * WEYL)`` and a
uniform in the open interval (0, 1) ``((r >> 12) + 0.5) * 2^-52``.  ``NOISE_STREAM`` and ``CHOICE_STREAM`` are the two
purposes; the sampler's uniform uses 0x5851F42D4C957F2D, so the three are independent for one ``(seed, env)``.  Draw indices of
the noise stream, for slot ``k`` and try ``j`` (0..15): ``64 k + 3 j + {0, 1, 2}`` = ``u0`` (Box-Muller radius), ``u1`` (its
angle), ``u2`` (the accept test); ``64 k + 48`` = ``u_b``, the boost of ``alpha < 1``.  The choice uses draw 0 of its stream.

Noise, for an active env whose model has epsilon > 0, ``n = clamp(n_cand, 1, width)``: ``eta ~ Dirichlet(alpha)`` over the n
candidates, ``s = p_0 + .. + p_{n-1}`` in slot order, ``p'_k = (1 - epsilon) p_k + epsilon s eta_k`` in float64, rounded once to
fp32: the candidates' prior mass is kept, so ``c_puct`` means the same with noise on and off.  ``Gamma(alpha)`` of slot k is
Marsaglia-Tsang: ``a' = alpha + 1 if alpha < 1 else alpha``, ``d = a' - 1/3``, ``c = 1 / sqrt(9 d)``; per try
``x = sqrt(-2 ln u0) cos(2 pi u1)``, ``t = 1 + c x``, ``v = t t t``, rejected if ``v <= 0``, accepted if
``ln u2 < 0.5 x x + d - d v + d ln v``; ``g = d v``, or ``d`` after 16 rejections, times ``exp(ln(u_b) / alpha)`` for
``alpha < 1``.  ``eta_k = g_k / sum g`` (slot order), ``1 / n`` where the sum is not above 0 or not finite.

Choice, behind the last simulation, with ``best`` the most visited root slot as always: where the env's game ply lies below
its model's ``sample_plies``, ``total = sum_{k<n} N_k``, ``x = ((r_0 >> 32) * total) >> 32`` and the played slot is the first
``k`` whose running sum of ``N`` exceeds ``x`` (a slot without visits is never drawn); elsewhere it is ``best``.
"""
from __future__ import annotations

import math
import struct
from dataclasses import dataclass
from typing import ClassVar, List, Optional, Tuple

import numpy as np
import torch

from ._forked_rows import check_int, controls_rows, table_of
from .sampling import MAX_OPENING_PLIES, _M64, _mix

__all__ = ["MctsExploration", "explore_table", "explore_controls", "arena_mcts_explore", "noise_stream",
           "stream_draw", "draw_uniform", "dirichlet_gammas_host", "root_noise_host", "visit_choice_host", "NOISE_STREAM",
           "CHOICE_STREAM", "MAX_SAMPLE_PLIES", "MIN_ALPHA", "MAX_ALPHA", "FLAG_SAMPLED", "FLAG_DIVERGED"]

NOISE_STREAM = 0x2545F4914F6CDD1D           # kXpNoise of csrc/mcts_explore.h
CHOICE_STREAM = 0xD1342543DE82EF95          # kXpChoice
WEYL = 0x9E3779B97F4A7C15                   # kKaWeyl of csrc/common.h
MAX_SAMPLE_PLIES = MAX_OPENING_PLIES
MIN_ALPHA, MAX_ALPHA = 0.01, 100.0
FLAG_SAMPLED, FLAG_DIVERGED = 16, 32        # record 0, bits 4 and 5
_TRIES, _SLOT_DRAWS, _BOOST_DRAW = 16, 64, 48


@dataclass(frozen=True)
class MctsExploration:
    """One model's exploration controls.  ``noise_fraction`` 0 is no noise, ``sample_plies`` 0 no drawn move."""
    noise_fraction: float = 0.0
    noise_alpha: float = 0.0
    sample_plies: int = 0

    OFF: ClassVar["MctsExploration"]

    def __post_init__(self) -> None:
        for name in ("noise_fraction", "noise_alpha"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v):
                raise ValueError(f"{name} must be a finite number, got {v!r}")
            object.__setattr__(self, name, float(v))
        if not 0.0 <= self.noise_fraction <= 1.0:
            raise ValueError(f"noise_fraction must lie in [0, 1], got {self.noise_fraction!r}")
        if self.noise_fraction > 0 and not MIN_ALPHA <= self.noise_alpha <= MAX_ALPHA:
            raise ValueError(f"noise_alpha must lie in [{MIN_ALPHA}, {MAX_ALPHA}] when noise_fraction is above 0, got "
                             f"{self.noise_alpha!r}")
        if self.noise_fraction == 0 and not 0.0 <= self.noise_alpha <= MAX_ALPHA:
            raise ValueError(f"noise_alpha must lie in [0, {MAX_ALPHA}], got {self.noise_alpha!r}")
        object.__setattr__(self, "sample_plies", check_int("sample_plies", self.sample_plies, 0, MAX_SAMPLE_PLIES))

    def row(self) -> np.ndarray:
        """The table row: fp32 noise_fraction, fp32 noise_alpha, int32 sample_plies, a reserved zero, as four int32."""
        return np.frombuffer(struct.pack("<ffii", self.noise_fraction, self.noise_alpha, self.sample_plies, 0),
                             dtype=np.int32).copy()


MctsExploration.OFF = MctsExploration()


def explore_table(controls, K: int) -> np.ndarray:
    """The ``(K, 4)`` int32 table (the two fractions bit-cast).  ``controls``: None (K rows ``OFF``), one
    ``MctsExploration`` (every model) or a sequence of exactly K."""
    return np.stack([r.row() for r in controls_rows(controls, K, MctsExploration, "mcts_explore")]).astype(np.int32, copy=False)


def arena_mcts_explore(mcts_explore, mcts, num_models: int) -> Optional[np.ndarray]:
    """``MatchArena``'s reading of ``mcts_explore=``: None stays None (nothing is allocated, no launch is added); everything
    else is a table of ``num_models`` rows -- refused without ``mcts=``: it is the visit-count search that is explored."""
    if mcts_explore is None:
        return None
    if mcts is None:
        raise ValueError("mcts_explore= needs mcts=: the noise goes into the root priors of the visit-count search and the "
                         "drawn move follows its visits")
    return explore_table(mcts_explore, num_models)


def explore_controls(controls, model_of) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """Per row ``(epsilon, alpha, sample_plies)`` as the kernels read them from the table (``controls``: an
    ``MctsExploration``, a sequence of them or a (K, 4) table): the fp32 values as float64; a row with a word out of range
    and a model outside ``[0, K)`` read as off."""
    table = table_of(controls, None, explore_table, "mcts_explore")
    mo = np.asarray(torch.as_tensor(model_of).cpu().numpy(), np.int64).reshape(-1)
    eps, alpha, plies = np.zeros(mo.shape[0]), np.zeros(mo.shape[0]), np.zeros(mo.shape[0], np.int64)
    for b, m in enumerate(mo):
        if not 0 <= m < table.shape[0]:
            continue
        e, a = (np.float32(x) for x in table[m, :2].view(np.float32))
        s = int(table[m, 2])
        ok = 0 <= e <= 1 and (e == 0 or np.float32(MIN_ALPHA) <= a <= np.float32(MAX_ALPHA)) and 0 <= s <= MAX_SAMPLE_PLIES
        if ok:                                                  # (a NaN fails every comparison)
            eps[b], alpha[b], plies[b] = float(e), float(a) if e > 0 else 0.0, s
    return eps, alpha, plies


# ---------------------------------------------------------------------------------------------- the draws
def noise_stream(seed: int, env: int, purpose: int = NOISE_STREAM) -> int:
    """``h`` of ``(seed, env)`` for ``purpose``."""
    return _mix((int(seed) & _M64) ^ _mix((int(env) + purpose) & _M64))


def stream_draw(h: int, i: int) -> int:
    """Draw ``i`` of the stream ``h``: 64 bits."""
    return _mix((h + i * WEYL) & _M64)


def draw_uniform(r: int) -> float:
    """The uniform in the open interval (0, 1) of a draw (exact in float64)."""
    return ((r >> 12) + 0.5) * 2.0 ** -52


def dirichlet_gammas_host(seed: int, env: int, n: int, alpha: float) -> Tuple[List[float], float]:
    """The ``n`` Gamma(alpha) values of ``(seed, env)`` before normalising, and the margin: the smallest distance by which
    any accept test (``ln u2`` against its bound) or any sign test (``1 + c x`` against 0, the sign of ``v``) of them was
    decided."""
    h = noise_stream(seed, env)
    a1 = alpha + 1.0 if alpha < 1.0 else alpha
    d = a1 - 1.0 / 3.0
    c = 1.0 / math.sqrt(9.0 * d)
    out, margin = [], math.inf
    for k in range(n):
        g = d
        for j in range(_TRIES):
            i = k * _SLOT_DRAWS + 3 * j
            u0, u1, u2 = (draw_uniform(stream_draw(h, i + x)) for x in range(3))
            x = math.sqrt(-2.0 * math.log(u0)) * math.cos(6.283185307179586 * u1)
            t = 1.0 + c * x
            v = t * t * t
            margin = min(margin, abs(t))
            if v <= 0.0:
                continue
            bound = 0.5 * x * x + d - d * v + d * math.log(v)
            margin = min(margin, abs(math.log(u2) - bound))
            if math.log(u2) < bound:
                g = d * v
                break
        if alpha < 1.0:
            g = g * math.exp(math.log(draw_uniform(stream_draw(h, k * _SLOT_DRAWS + _BOOST_DRAW))) / alpha)
        out.append(g)
    return out, margin


def root_noise_host(seed: int, priors, n_cand, active, controls, model_of) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The float64 restatement of ``ka_mcts_root_noise``: ``priors`` (B, W) fp32 as the fork wrote them, ``n_cand`` (B,),
    ``active`` (B,) bool (flag bit 0 of record 0), ``controls`` an ``MctsExploration``, a sequence of them or a (K, 4) table,
    ``model_of`` (B,) (None: model 0).  Returns ``(noised, eta, margin)``: the priors after the noise (B, W) fp32 -- the
    input's bits in every cell the kernel does not write --, eta (B, W) float64 (0 in the unused cells and the rows not
    noised) and per row the smallest distance by which any test of its draw was decided (inf for a row not noised)."""
    p = np.ascontiguousarray(torch.as_tensor(priors).cpu().numpy()).astype(np.float32, copy=True)
    B, W = p.shape
    n_cand = np.asarray(torch.as_tensor(n_cand).cpu().numpy(), np.int64).reshape(B)
    act = np.asarray(torch.as_tensor(active).cpu().numpy()).astype(bool).reshape(B)
    eps, alpha, _ = explore_controls(controls, np.zeros(B, np.int64) if model_of is None else model_of)
    eta, margin = np.zeros((B, W)), np.full(B, np.inf)
    for b in range(B):
        if not act[b] or not eps[b] > 0:
            continue
        n = min(max(int(n_cand[b]), 1), W)
        g, margin[b] = dirichlet_gammas_host(seed, b, n, float(alpha[b]))
        s = gs = 0.0
        for k in range(n):                                     # slot order: part of the contract
            s += float(p[b, k])
            gs += g[k]
        for k in range(n):
            eta[b, k] = g[k] / gs if gs > 0.0 and math.isfinite(gs) else 1.0 / n
        for k in range(n):
            p[b, k] = np.float32((1.0 - eps[b]) * float(p[b, k]) + eps[b] * s * eta[b, k])
    return p, eta, margin


def visit_choice_host(seed: int, visits, n_cand, game_ply, controls, model_of) -> Tuple[np.ndarray, np.ndarray]:
    """The restatement of the choice of ``ka_mcts_advance_explore``, exact: ``visits`` (B, W) int the root visits, ``n_cand``
    (B,), ``game_ply`` (B,), controls and ``model_of`` as ``root_noise_host``.  Returns ``(slot, sampled)``: the played slot
    (B,) and whether it was drawn (B,) bool; where it was not, the slot is the first maximum of the visits."""
    N = np.asarray(torch.as_tensor(visits).cpu().numpy(), np.int64)
    B, W = N.shape
    n_cand = np.asarray(torch.as_tensor(n_cand).cpu().numpy(), np.int64).reshape(B)
    ply = np.asarray(torch.as_tensor(game_ply).cpu().numpy(), np.int64).reshape(B)
    _, _, plies = explore_controls(controls, np.zeros(B, np.int64) if model_of is None else model_of)
    slot, sampled = np.zeros(B, np.int64), np.zeros(B, bool)
    for b in range(B):
        n = min(max(int(n_cand[b]), 1), W)
        best = 0
        for k in range(1, n):
            if N[b, k] > N[b, best]:                           # ties keep the lower slot
                best = k
        slot[b] = best
        if 0 <= ply[b] < plies[b]:
            total = int(N[b, :n].sum())
            x = ((stream_draw(noise_stream(seed, b, CHOICE_STREAM), 0) >> 32) * total) >> 32
            run = 0
            for k in range(n):
                run += int(N[b, k])
                if run > x:
                    slot[b] = k
                    break
            sampled[b] = True
    return slot, sampled
