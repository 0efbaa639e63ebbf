"""Inputs that tests/test_mcts_explore_cpu.py and tests/test_hip_mcts_explore.py share: the synthetic records the noise kernel
is run on alone, and the fixed seeds of the device tests.  The CPU file asserts the margin condition on exactly these inputs
(no accept test of their draws is decided by less than ``MARGIN``), the device file relies on it."""
import numpy as np

from keisei_amd.training.lookahead import REC_CAND, REC_FLAGS, REC_NCAND, lookahead_words
from keisei_amd.training.mcts_explore import MctsExploration

MARGIN = 1e-9
POISON = np.int32(-559038737)                                 # 0xDEADBEEF
# env counts around the eight envs of a wave and the thirty-two of a block (one lane per (env, slot), eight lanes per env)
NOISE_B = (1, 7, 8, 9, 31, 32, 33, 257)
NOISE_W = (1, 3, 8)
ALPHA = {1: 1.0, 3: 3.0, 8: 0.15}                             # alpha = 1, above 1 and below 1 (the boosted draw)
EPSILON = 0.25
STEP_SEED, STEP_ENVS, STEP_W, STEP_ALPHA = 0x5EED0000BEEF, 16, 4, 0.15     # MctsSearch.step on a real env


def noise_seed(B, W):
    return 0x1234ABCD0000 + 1000 * B + W


def noise_controls(W):
    return [MctsExploration(EPSILON, ALPHA[W], 0), MctsExploration.OFF]


def noise_case(B, W):
    """Records (B, words) int32 as the fork would leave them, everything the fork does not define holding ``POISON``:
    ``n_cand`` sweeps 1..W, some rows are inactive, some belong to model 1 (off) and one to model -1."""
    rng = np.random.default_rng([811, B, W])
    model_of = rng.choice(np.array([0, 0, 0, 1], np.int32), B)
    active = rng.random(B) < 0.8
    active[0], model_of[0] = True, 0
    if B >= 7:
        model_of[1], active[1] = 1, True
        active[2], model_of[2] = False, 0
        model_of[B // 2], active[B // 2] = -1, True
    n_cand = (np.arange(B) % W + 1).astype(np.int32)
    priors = rng.random((B, W))
    priors = (priors / (priors.sum(1, keepdims=True) * rng.uniform(1.0, 1.5, (B, 1)))).astype(np.float32)
    rec = np.full((B, lookahead_words(W)), POISON, np.int32)
    rec[:, REC_FLAGS] = active
    rec[:, REC_NCAND] = n_cand
    for b in range(B):
        n = int(n_cand[b])
        rec[b, REC_CAND:REC_CAND + n] = rng.integers(0, 11259, n)
        rec[b, REC_CAND + W:REC_CAND + W + n] = priors[b, :n].view(np.int32)
    return dict(B=B, W=W, seed=noise_seed(B, W), ctl=noise_controls(W), model_of=model_of, active=active, n_cand=n_cand,
                priors=priors, rec=rec)
