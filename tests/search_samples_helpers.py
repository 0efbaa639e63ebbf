"""What the search-sample tests share: a hand-written script of plies for ``ka_search_sample_step`` with every expected word
stated from the script's own tables (not through the restatement under test), a seeded random script, and the float64
reference of ``ka_policy_ce_soft``."""
import struct

import numpy as np
import torch

from keisei_amd.training.lookahead import REC_CAND, REC_FLAGS, REC_NCAND, lookahead_words
from keisei_amd.training.search_samples import META_WORDS, ROW_WORDS

E, R, T = 5, 3, 6
NAN = float("nan")
# per env, per ply: (active, n_cand before the cut to the width, model, mover's reward, terminated, truncated)
SCRIPT = (
    # env 0: a game won by the last mover (plies 0-1), then a second game in the same region whose last sample finds the
    # region full (ply 3: dropped, and the stored row 2 is still labelled: lost by the last mover), then an open game
    ((1, 2, 0, 0.0, 0, 0), (1, 3, 0, 1.0, 1, 0), (1, 8, 0, 0.0, 0, 0), (1, 1, 0, -1.0, 1, 0), (1, 2, 0, 0.0, 0, 0), (0, 2, 0, 0.0, 0, 0)),
    # env 1: a game lost by the last mover over three plies fills the region; three more samples are dropped
    ((1, 3, 1, 0.0, 0, 0), (1, 2, 1, 0.0, 0, 0), (1, 3, 1, -1.0, 1, 0), (1, 1, 1, 0.0, 0, 0), (1, 1, 1, 0.0, 0, 0), (1, 1, 1, 0.0, 0, 0)),
    # env 2: a draw by truncation, then a game that ends on a NaN reward (a draw) with its last sample dropped
    ((1, 1, 0, 0.0, 0, 0), (1, 2, 0, 0.0, 0, 1), (1, 3, 0, 0.0, 0, 0), (1, 2, 0, NAN, 1, 0), (0, 1, 0, 0.0, 0, 0), (0, 1, 0, 0.0, 0, 0)),
    # env 3: inactive, then unseated (model -1), two samples of a game the last mover wins, no candidate, an open game
    ((0, 2, 1, 0.0, 0, 0), (1, 2, -1, 0.0, 0, 0), (1, 2, 1, 0.0, 0, 0), (1, 3, 1, 1.0, 1, 0), (1, 0, 1, 0.0, 0, 0), (1, 2, 1, 0.0, 0, 0)),
    # env 4: two samples of a game still open at the end
    ((1, 2, 0, 0.0, 0, 0), (1, 1, 0, 0.0, 0, 0), (0, 1, 0, 0.0, 0, 0), (0, 1, 0, 0.0, 0, 0), (0, 1, 0, 0.0, 0, 0), (0, 1, 0, 0.0, 0, 0)),
)
# per env: the rows the store must hold after the last ply, (ply written at, value word, move index, game number)
STORED = (
    ((0, 2, 0, 0), (1, 0, 1, 0), (2, 0, 0, 1)),
    ((0, 2, 0, 0), (1, 0, 1, 0), (2, 2, 2, 0)),
    ((0, 1, 0, 0), (1, 1, 1, 0), (2, 1, 0, 1)),
    ((2, 2, 2, 0), (3, 0, 3, 0), (5, -1, 1, 1)),
    ((0, -1, 0, 0), (1, -1, 1, 0)),
)
# per env: cursor, first row of the open game, dropped, moves of the open game, games finished
META = ((3, 3, 2, 2, 2), (3, 3, 3, 3, 1), (3, 3, 1, 2, 2), (3, 2, 0, 2, 1), (2, 0, 0, 6, 0))
# (env, ply) -> the meta after that ply, a few stations on the way
META_AT = {(0, 1): (2, 2, 0, 0, 1), (0, 3): (3, 3, 1, 0, 2), (3, 1): (0, 0, 0, 2, 0), (3, 3): (2, 2, 0, 0, 1), (2, 3): (3, 3, 1, 0, 2)}


def mover(t, e):
    return (t + e) & 1


def action(t, e):
    return 1000 + 17 * t + e


def material(t, e):
    return 19 * t - 38 * (e % 3)


def candidate(t, e, j):
    return 100 * t + 10 * e + j + 1


def visits(t, e, j):
    return 1 + (t + e + j) % 5


def f32_bits(x) -> int:
    return struct.unpack("<I", struct.pack("<f", x))[0]


def observation(t, e) -> np.ndarray:
    """channel 0: one square set to 1; channel 3: a constant plane; channel 49: the two corner squares; the rest empty"""
    obs = np.zeros((50, 81), np.float32)
    obs[0, (7 * t + e) % 81] = 1.0
    obs[3, :] = 0.25 * (e + 1)
    obs[49, 0] = obs[49, 80] = 1.0
    return obs.reshape(-1)


def script_ply(t: int, W: int, script=SCRIPT) -> dict:
    """The inputs of ply t at width W, as numpy arrays over the envs"""
    n = len(script)
    rec = np.zeros((n, lookahead_words(W)), np.int32)
    vis = np.zeros((n, W), np.int32)
    ply = dict(obs=np.stack([observation(t, e) for e in range(n)]), players=np.array([mover(t, e) for e in range(n)], np.uint8),
               actions=np.array([action(t, e) for e in range(n)], np.int64),
               material=np.array([material(t, e) for e in range(n)], np.int32), model_of=np.zeros(n, np.int32),
               rewards=np.zeros(n, np.float32), terminated=np.zeros(n, np.uint8), truncated=np.zeros(n, np.uint8))
    for e in range(n):
        active, ncand, model, reward, tm, tr = script[e][t]
        rec[e, REC_FLAGS] = active | 4                                       # (another flag bit beside bit 0)
        rec[e, REC_NCAND] = min(ncand, W)
        rec[e, REC_CAND:REC_CAND + W] = [candidate(t, e, j) for j in range(W)]
        vis[e] = [visits(t, e, j) for j in range(W)]                         # (the slots behind n_cand hold stale counts)
        ply["model_of"][e], ply["rewards"][e], ply["terminated"][e], ply["truncated"][e] = model, reward, tm, tr
    ply.update(records=rec, root_visits=vis)
    return ply


def expected_row(t, e, W, value, move, game) -> np.ndarray:
    """The 216 words of the sample of ply t in env e, from the script's tables"""
    row = np.zeros(ROW_WORDS, np.uint32)
    sq = (7 * t + e) % 81
    row[sq >> 5] = 1 << (sq & 31)
    row[150] = 0x3F800000
    row[9:12] = (0xFFFFFFFF, 0xFFFFFFFF, 0x0001FFFF)
    row[153] = f32_bits(0.25 * (e + 1))
    row[147:150] = (0x00000001, 0, 0x00010000)
    row[199] = 0x3F800000
    row[200] = action(t, e)
    row[201] = value & 0xFFFFFFFF
    row[202] = f32_bits(np.float32(material(t, e)) / np.float32(76.0))
    active, ncand, model, *_ = SCRIPT[e][t]
    for j in range(min(ncand, W)):
        row[204 + j] = candidate(t, e, j) | (visits(t, e, j) << 16)
    row[212:216] = (model | (mover(t, e) << 16), move, e, game)
    return row


def expected_store(W):
    rows = np.zeros((E, R, ROW_WORDS), np.uint32)
    for e, stored in enumerate(STORED):
        for r, (t, value, move, game) in enumerate(stored):
            rows[e, r] = expected_row(t, e, W, value, move, game)
    return rows, np.array(META, np.int32)


def random_script(seed: int, envs: int = E, plies: int = 14):
    """A seeded script in SCRIPT's form: short games, idle and unseated envs, empty candidate lists, every reward sign"""
    g = np.random.default_rng(seed)
    out = []
    for _ in range(envs):
        row = []
        for _ in range(plies):
            done = g.random() < 0.3
            row.append((int(g.random() < 0.8), int(g.integers(0, 9)), int(g.integers(-1, 3)),
                        float(g.choice([0.0, 1.0, -1.0, NAN])) if done else 0.0, int(done and g.random() < 0.6),
                        0))
            a, n, m, rw, tm, _ = row[-1]
            row[-1] = (a, n, m, rw, tm, int(done and not tm))
        out.append(tuple(row))
    return tuple(out)


# ---------------------------------------------------------------------------------------------- the soft cross-entropy
def soft_ce_ref(logits, actions, weights, w_policy: float, dt: torch.dtype, gscale: float = 1.0) -> dict:
    """``ka_policy_ce_soft`` by autograd in ``dt``: rowloss = sum_k w_k (lse - z[a_k]) over the used slots (w_k > 0), dlogits
    the gradient of ``w_policy * gscale * sum(rowloss)``.  The rows are valid (the flag cases are tested apart)."""
    lg = logits.to(dt).clone().requires_grad_(True)
    w = weights.to(dt)
    used = weights > 0
    a = torch.where(used, actions.long(), torch.zeros_like(actions.long()))
    nlp = -torch.log_softmax(lg, dim=-1).gather(1, a)
    rows = (torch.where(used, w, torch.zeros_like(w)) * nlp).sum(1)
    (dl,) = torch.autograd.grad(w_policy * gscale * rows.sum(), lg)
    return {"rowloss": rows.detach(), "dlogits": dl}


def dense_targets(actions, weights, A: int) -> torch.Tensor:
    """(B, A) float64 probabilities of the slots (duplicates add)"""
    used = weights > 0
    out = torch.zeros(actions.shape[0], A, dtype=torch.float64)
    out.scatter_add_(1, torch.where(used, actions.long(), torch.zeros_like(actions.long())),
                     torch.where(used, weights.double(), torch.zeros_like(weights.double())))
    return out


SOFT_B = 16
ONE_SLOT, ALL_USED, DUPLICATE, ZERO_INVALID, LAST_ACTION = (0, 5), (1, 6), (2, 7), (3, 8), (4, 9)    # rows of each kind


def soft_case(A: int, K: int, scale: float = 3.0):
    """``(logits (16, A), actions (16, K) int32, weights (16, K) fp32)``: rows 0 and 5 one slot of weight 1 (the others
    unused), 1 and 6 every slot used, 2 and 7 a duplicated action (K > 1), 3 and 8 a zero-weight slot with an invalid action,
    4 and 9 action A - 1, the rest random with random unused slots; at A = 1 every slot names action 0."""
    g = torch.Generator().manual_seed(1000 * A + K)
    logits = (scale * torch.randn(SOFT_B, A, generator=g)).float()
    actions = torch.randint(0, A, (SOFT_B, K), generator=g).to(torch.int32)
    counts = torch.randint(1, 40, (SOFT_B, K), generator=g).float()
    keep = torch.rand(SOFT_B, K, generator=g) < 0.7
    keep[:, 0] = True
    for b in ALL_USED + DUPLICATE + LAST_ACTION:
        keep[b] = True
    for b in ONE_SLOT:
        keep[b] = False
        keep[b, b % K] = True
    counts = torch.where(keep, counts, torch.zeros_like(counts))
    weights = (counts / counts.sum(1, keepdim=True)).float()
    for b in ONE_SLOT:
        assert float(weights[b, b % K]) == 1.0
    if K > 1:
        for b in DUPLICATE:
            actions[b, K - 1] = actions[b, 0]
        for b in ZERO_INVALID:
            weights[b, 1] = 0.0
            actions[b, 1] = A + 5 if b == ZERO_INVALID[0] else -3
            weights[b] = weights[b] / weights[b].sum()
    for b in LAST_ACTION:
        actions[b, 0] = A - 1
    return logits, actions, weights
