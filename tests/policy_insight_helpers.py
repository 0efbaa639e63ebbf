"""Shared by the policy-insight tests: a float64 numpy restatement of the reference's showcase lines (runner.py:151-173,
heatmap.py:40-49, inference.py:95), an independent USI decode of the spatial action space, and the rows the tests use.
Nothing here imports the code under test."""
import functools
import math

import numpy as np

A = 81 * 139
SLOTS = 139
HEAT = 132
RTOL, ATOL = 1e-4, 5e-5            # the project's fp32 output tolerance (README)
_DIRS = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))     # N NE E SE S SW W NW
_HAND = "PLNSGBR"


def _sq(sq: int) -> str:
    return f"{9 - sq % 9}{'abcdefghi'[sq // 9]}"


def usi(action: int, colour: int):
    """USI of a spatial action played by `colour`, or None where it points off the board."""
    frm, slot = divmod(int(action), SLOTS)
    r, c = divmod(frm, 9)
    flip = (lambda q: 80 - q) if colour else (lambda q: q)
    if slot >= HEAT:
        return f"{_HAND[slot - HEAT]}*{_sq(flip(frm))}"
    if slot < 128:
        d, dist = (slot % 64) // 8, slot % 8 + 1
        tr, tc, promote = r + _DIRS[d][0] * dist, c + _DIRS[d][1] * dist, slot >= 64
    else:
        k = slot - 128
        tr, tc, promote = r - 2, c + (1 if k >> 1 else -1), bool(k & 1)
    if not (0 <= tr < 9 and 0 <= tc < 9):
        return None
    return _sq(flip(frm)) + _sq(flip(tr * 9 + tc)) + ("+" if promote else "")


def bf16_round(x: np.ndarray) -> np.ndarray:
    """fp32 -> the nearest bf16 (ties to even), back in fp32."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def oracle_row(logits, legal_mask, action, vlogits, temperature: float, top_k: int) -> dict:
    """One row in float64.  The distribution is runner.py:151-163 word for word; the candidates are ordered by raw logit
    (descending, equal logits by lower action) and the rank counts raw logits, as the issue defines them."""
    policy_logits = np.asarray(logits, dtype=np.float64)
    legal = np.flatnonzero(legal_mask)
    out = {"n_legal": int(legal.size)}
    mask = np.full(policy_logits.shape, -1e9)
    mask[legal] = 0.0
    masked_logits = policy_logits + mask
    scaled_logits = masked_logits / temperature
    legal_logits = scaled_logits[legal]
    legal_probs = np.exp(legal_logits - legal_logits.max())
    legal_probs = legal_probs / legal_probs.sum()
    probs = np.zeros_like(scaled_logits)
    probs[legal] = legal_probs
    out["probs"] = probs
    nz = legal_probs[legal_probs > 0]
    out["entropy"] = float(-(nz * np.log(nz)).sum())
    ok = 0 <= action < A and bool(legal_mask[action])
    out["legal_action"] = ok
    out["chosen_probability"] = float(probs[action]) if ok else 0.0
    out["chosen_rank"] = int((policy_logits[legal] > policy_logits[action]).sum()) if ok else -1
    order = legal[np.lexsort((legal, -policy_logits[legal]))][:top_k]
    out["top_actions"] = [int(a) for a in order] + [-1] * (top_k - len(order))
    out["top_probabilities"] = [float(probs[a]) for a in order] + [0.0] * (top_k - len(order))
    heat = np.zeros(HEAT)
    if ok:
        frm, slot = divmod(int(action), SLOTS)
        if slot < HEAT:
            heat[:] = probs[frm * SLOTS:frm * SLOTS + HEAT]
        else:
            heat[:81] = probs[slot::SLOTS]
    out["heat"] = heat
    if vlogits is None:
        out["win_probability"] = 0.0
    else:
        v = np.asarray(vlogits, dtype=np.float64)
        e = np.exp(v - v.max())
        out["win_probability"] = float(e[0] / e.sum())
    return out


def runner_candidates(o: dict, colour: int) -> list:
    """runner.py:169-173 over the oracle's candidates, with the real USI of each."""
    return [{"action": a, "probability": round(float(p), 4), "usi": usi(a, colour) or "?"}
            for a, p in zip(o["top_actions"], o["top_probabilities"]) if a >= 0 and p > 0.001]


def build_heatmap(chosen_usi: str, legal_with_usi, probs) -> dict:
    """heatmap.py:40-49."""
    target = chosen_usi[:2]
    out = {}
    for idx, u in legal_with_usi:
        if u[:2] != target:
            continue
        prob = probs.get(idx)
        if prob is None or not math.isfinite(prob) or prob <= 0.0:
            continue
        out[u] = float(prob)
    return out


# ---------------------------------------------------------------------------------------------- rows
PAWN_PUSH = 56 * SLOTS + 0            # 7g7f for black, 3c3d for white
DROP_SILVER = 40 * SLOTS + HEAT + 3   # S*5e
KNIGHT = 60 * SLOTS + 130             # from 3g, two up and one right, no promotion


@functools.lru_cache(maxsize=None)
def crafted_rows():
    """(logits (5, A) fp32, legal (5, A) bool, actions (5,), value logits (5, 3), players (5,)): one legal move; every action
    legal; a chosen drop; a chosen knight slot; bitwise-equal top logits."""
    rng = np.random.default_rng(20261019)
    logits = (rng.standard_normal((5, A)) * 2.0).astype(np.float32)
    legal = np.zeros((5, A), dtype=bool)
    legal[0, PAWN_PUSH] = True
    legal[1, :] = True
    drops = [sq * SLOTS + HEAT + 3 for sq in (0, 13, 40, 41, 80)]
    legal[2, drops + [40 * SLOTS + HEAT + 1, 40 * SLOTS + 5, 12 * SLOTS + 64, 3]] = True
    legal[3, [60 * SLOTS + s for s in (0, 7, 64, 128, 129, 130, 131)] + [61 * SLOTS + 130, 59 * SLOTS + 130]] = True
    tied = [9000, 17, 4242, 11258]
    legal[4, tied + [0, 300, 301, 5000, 7000, 10000]] = True
    logits[4, tied] = np.float32(1.7320508)
    logits[4, [300, 301]] = np.float32(-0.25)          # a second tie, below the first
    logits[4, [0, 5000, 7000, 10000]] = np.array([-3.0, 0.5, -1.0, 1.0], dtype=np.float32)
    actions = np.array([PAWN_PUSH, 56 * SLOTS + 3, DROP_SILVER, KNIGHT, 4242], dtype=np.int64)
    vlogits = rng.standard_normal((5, 3)).astype(np.float32)
    players = np.array([0, 1, 1, 0, 1], dtype=np.uint8)
    return logits, legal, actions, vlogits, players


@functools.lru_cache(maxsize=None)
def seeded_rows(rows: int = 67, seed: int = 7):
    """`rows` random rows with 1..200 legal actions; row 10's action is illegal, row 11's negative, row 12's past A."""
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((rows, A)) * 3.0).astype(np.float32)
    legal = np.zeros((rows, A), dtype=bool)
    actions = np.zeros(rows, dtype=np.int64)
    for b in range(rows):
        idx = rng.choice(A, size=int(rng.integers(1, 201)), replace=False)
        legal[b, idx] = True
        actions[b] = idx[int(rng.integers(0, idx.size))]
    if rows > 12:
        actions[10] = int(np.flatnonzero(~legal[10])[5])
        actions[11] = -5
        actions[12] = A + 3
    vlogits = rng.standard_normal((rows, 3)).astype(np.float32)
    players = rng.integers(0, 2, size=rows).astype(np.uint8)
    return logits, legal, actions, vlogits, players


@functools.lru_cache(maxsize=None)
def oracle_of(which: str, bf16: bool, temperature: float, top_k: int = 8) -> tuple:
    """The oracle of every row of `crafted_rows()` / `seeded_rows()`, computed once per (rows, dtype, temperature)."""
    logits, legal, actions, vlogits, _ = crafted_rows() if which == "crafted" else seeded_rows()
    if bf16:
        logits = bf16_round(logits)
    return tuple(oracle_row(logits[b], legal[b], int(actions[b]), vlogits[b], temperature, top_k) for b in range(logits.shape[0]))


def check_rows(res, oracle, top_k: int, what: str = "") -> None:
    """`res`: anything with the PolicyInsight fields as numpy arrays; `oracle`: `oracle_of(...)` at top_k >= this top_k."""
    for b, o in enumerate(oracle):
        tag = f"{what} row {b}"
        assert int(res["n_legal"][b]) == o["n_legal"], tag
        assert int(res["chosen_rank"][b]) == o["chosen_rank"], tag
        assert bool(int(res["flags"][b]) & 4) == o["legal_action"] and int(res["flags"][b]) & 1, tag
        assert [int(a) for a in res["top_actions"][b]] == o["top_actions"][:top_k], tag
        np.testing.assert_allclose(res["top_probabilities"][b], o["top_probabilities"][:top_k], rtol=RTOL, atol=ATOL, err_msg=tag)
        for key in ("chosen_probability", "entropy", "win_probability"):
            np.testing.assert_allclose(float(res[key][b]), o[key], rtol=RTOL, atol=ATOL, err_msg=f"{tag} {key}")
        np.testing.assert_allclose(res["heat"][b], o["heat"], rtol=RTOL, atol=ATOL, err_msg=f"{tag} heat")
        assert not np.any(res["heat"][b][o["heat"] == 0.0]), tag          # illegal members and the rest are exactly 0


def as_numpy(pi) -> dict:
    """A PolicyInsight as numpy arrays."""
    keys = ("chosen_probability", "entropy", "n_legal", "chosen_rank", "win_probability", "top_actions", "top_probabilities",
            "heat", "flags", "records", "nan_flag")
    return {k: getattr(pi, k).detach().cpu().numpy() for k in keys}
