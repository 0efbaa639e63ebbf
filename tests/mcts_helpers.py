"""Synthetic worlds for the visit-count search: what tests/test_mcts_cpu.py (with the restatement as the chooser) and
tests/test_hip_mcts.py (with ka_mcts_advance as the chooser) walk, simulation by simulation.

A world is, for E simulations of width W over B rows, what every fork *would* find wherever the chooser sends it: candidate
counts, candidate actions, priors from {0, 0.5, 1}, value-logit triples whose P(L) - P(W) is one of ``QS`` (pairwise at least
0.05 apart), done flags and rewards.  Row 0 is an inactive root and row 1 a root with a single candidate.  Two models search it
with different ``simulations`` and ``c_puct``.

The gap condition.  ka_mcts_advance scores in fp32, the restatement in float64, so a selection whose two best scores lie closer
than fp32 can tell apart could go either way.  ``gap_violations`` lists the selections whose two best scores are neither
computed from bit-identical operand triples (S, N, P) -- a tie in both arithmetics, the lower slot wins -- nor at least
``GAP`` apart.  PUCT drives the scores of a node's best children together by design, so a world of 64 generic rows has such
selections sooner or later; ``make_world`` keeps them away by drawing a row again until it has none, not by leaving
selections out (tests/test_mcts_cpu.py asserts the condition for the worlds of ``SEEDS``, the ones the device walks)."""
import numpy as np

from keisei_amd.shogi_gym import ACTION_SPACE
from keisei_amd.training import MctsControls, MctsRestatement, search_leaf_q, search_records
from keisei_amd.training.lookahead import REC_CAND

QS = (-0.6, -0.45, -0.2, 0.05, 0.1, 0.25, 0.35, 0.5, 0.7)      # every |q| differs from every other by at least 0.05
GAP = 1e-3
C_PUCT = (0.0371, 0.25)
SHAPES = [(1, 1), (3, 5), (8, 64)]
SEEDS = {(W, E): 70 + W for W, E in SHAPES}
B = 64


def triples(qs):
    """value logits whose P(L) - P(W) is q, with P(D) = 0.2"""
    return np.array([[np.log((0.8 - q) / 2), np.log(0.2), np.log((0.8 + q) / 2)] for q in qs], np.float32)


def controls(W, E):
    """model 0 searches all E simulations, model 1 about a third of them with another c_puct"""
    return [MctsControls(W, E, C_PUCT[0]), MctsControls(W, max(1, (E + 2) // 3), C_PUCT[1])]


def _row_world(W, E, seed, row, attempt, model, p_done=0.15, p_full=0.8):
    """the world of one row (B = 1), drawn from its own generator"""
    rng = np.random.default_rng([seed, row, attempt])
    vl = triples(QS)[rng.integers(0, len(QS), (E, 1, W))]
    done = rng.random((E, 1, W)) < p_done
    rewards = (rng.integers(-1, 2, (E, 1, W)) * done).astype(np.float32)
    priors = (rng.integers(0, 3, (E, 1, W)) / 2).astype(np.float32)
    n_all = rng.integers(0, W + 1, (E, 1))
    n_all[1:][rng.random((E - 1, 1)) < p_full] = W                # most forks find every candidate
    n_all[0] = [0, 1, W, W][row] if row < 4 else max(int(n_all[0, 0]), 1)
    cands = rng.integers(0, ACTION_SPACE, (E, 1, W))
    sampled = np.where(rng.random(1) < 0.5, cands[0, :, 0], 0).astype(np.int64)
    return dict(W=W, E=E, B=1, vl=vl, done=done, rewards=rewards, priors=priors, n_all=n_all, cands=cands,
                ctl=controls(W, E), model_of=np.array([model], np.int32), sampled=sampled)


def make_world(W, E, seed, n_rows=B, margin=1.1):
    """The world of ``seed``.  Every row is drawn from its own generator and walked alone with the restatement as the chooser
    (rows do not see each other); a row with a selection closer than ``margin * GAP`` that is no exact tie is drawn again --
    the resampling the gap condition asks for, done where the world is made, so that both test files walk the same rows.  The
    margin keeps a gap that the kernel's fp32 leaf q move by an ulp on the right side of GAP."""
    global GAP
    models = np.random.default_rng(seed).integers(0, 2, n_rows)
    rows = []
    for row in range(n_rows):
        for attempt in range(200):
            rw = _row_world(W, E, seed, row, attempt, int(models[row]))
            gap, GAP = GAP, margin * GAP
            try:
                clean = not walk_restatement(rw)[1]
            finally:
                GAP = gap
            if clean:
                break
        else:
            raise AssertionError(f"no world without a close selection for row {row} of seed {seed}")
        rows.append(rw)
    cat = lambda k: np.concatenate([r[k] for r in rows], axis=0 if rows[0][k].ndim == 1 else 1)  # noqa: E731
    return dict(W=W, E=E, B=n_rows, ctl=controls(W, E),
                **{k: cat(k) for k in ("vl", "done", "rewards", "priors", "n_all", "cands", "model_of", "sampled")})


def record_of(world, t, on):
    """record (t, .) as the fork would write it for the rows that are ``on`` (B,) bool: candidates and priors, no q yet"""
    n_t = np.where(on, world["n_all"][t], 0)
    return search_records(n_t[None], world["priors"][t][None], None, world["cands"][t][None])[0].numpy()


def walk(world, advance):
    """Simulation by simulation: ``advance(t, record_t)`` is the chooser; it returns ``fork_next`` (B,) bool, the rows
    whose simulation t + 1 forks."""
    on = np.ones(world["B"], bool)
    for t in range(world["E"]):
        on = np.asarray(advance(t, record_of(world, t, on)), bool)


def walk_restatement(world):
    """The world walked with the restatement itself as the chooser (the leaf q rounded to fp32 as a record holds them).
    Returns the restatement and the gap violations ``(t, row, level)`` of every selection made on the way."""
    W, E = world["W"], world["E"]
    r = MctsRestatement(world["ctl"], world["model_of"], world["B"], W, E)
    bad = []

    def advance(t, rec):
        q, _ = search_leaf_q(world["vl"][t], world["rewards"][t], world["done"][t])
        rec.view(np.float32)[:, REC_CAND + 2 * W:] = q.astype(np.float32)
        r.advance(rec, world["done"][t])
        for b, sel in enumerate(r.selections[-1]):
            bad.extend((t, b, v) for v in gap_violations(sel, r.N[b].reshape(-1), r.S32[b].reshape(-1), r.P[b].reshape(-1), W,
                                                              r.S[b].reshape(-1)))
        return r.fork_next

    walk(world, advance)
    return r, bad


def gap_violations(selection, N, S32, P, W, S64):
    """Of one row's selection (the levels ``(x, scores, chosen)``): the levels whose two best scores are neither of
    bit-identical (S, N, P) nor at least GAP apart.  ``N``, ``S32``, ``P``, ``S64`` (T * W,): the row's tree when it was
    made.  Identical means identical in both arithmetics: two fp32 sums may round to the same bits where the exact sums
    (which the float64 ones are, for a few fp32 terms) differ by 1e-8 -- a tie on the device and none in the restatement."""
    bad = []
    for x, scores, k in selection:
        if len(scores) < 2:
            continue
        order = np.argsort(-scores, kind="stable")
        a, b = x * W + int(order[0]), x * W + int(order[1])
        same = N[a] == N[b] and np.float32(S32[a]).tobytes() == np.float32(S32[b]).tobytes() and S64[a] == S64[b] and \
            np.float32(P[a]).tobytes() == np.float32(P[b]).tobytes()
        if not same and not scores[order[0]] - scores[order[1]] >= GAP:
            bad.append((x, scores.tolist(), k))
    return bad
