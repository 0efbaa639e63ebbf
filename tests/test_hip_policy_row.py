"""The candidate order of csrc/policy_row.h through its three callers: ka_policy_insight (top_k 8, temperature 1),
ka_lookahead_fork in its "candidates and priors only" mode (width 8, prior weight 0, skip 0, no env or child rows) and a
greedy row of ka_policy_sample_ctl, on 12 crafted rows over the whole spatial action space, fp32 and bf16.  The insight's
top actions and the fork's candidates are equal slot by slot, -1 for unused slots included; the greedy action is slot 0 of
both; the fork's priors are the insight's probabilities within the project's fp32 output tolerance; and a plain numpy
restatement of the order (finite legal logits by logit descending, then action ascending) is the third witness.

The rows are those where a copy of the order could drift: equal logits on actions whose mask words belong to different
waves, inside one word, across the first and the last word, on every action of the row; a tie straddling slot 8; fewer than
8 legal actions; the last bit of the last word alone; illegal actions with the largest logits; legal -inf; legal NaN.  Every
row's first 8 of the order are finite, so the three kernels agree whatever their own rule for a legal -inf.  A legal NaN
makes the insight's normaliser NaN by that kernel's definition (it raises flags[0] and every probability of the row is
NaN), while the fork passes a NaN over: on that one row the priors are held to the numpy softmax over the other legal
logits, and the insight's probabilities are required to be NaN."""
import functools

import numpy as np
import pytest
import torch

from keisei_amd import _lib
from keisei_amd.shogi_gym import ACTION_SPACE, MASK_WORDS
from keisei_amd.training import SamplingControls, controls_table
from keisei_amd.training.lookahead import REC_CAND, REC_NCAND, LookaheadControls, lookahead_table, lookahead_words
from keisei_amd.training.policy_insight import HEAT_WORDS, REC_NLEGAL, REC_TOP, insight_words
from policy_insight_helpers import ATOL, RTOL, bf16_round

pytestmark = pytest.mark.gpu
DEV = "cuda"
A, K = ACTION_SPACE, 8
NAN_ROW = 4
DTYPES = pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])


@functools.lru_cache(maxsize=None)
def _rows():
    """(logits (12, A) fp32, legal (12, A) bool).  Every crafted value is exact in bf16; the seeded background is not, so its
    bf16 rounding adds ties of its own."""
    assert A == 11259
    rng = np.random.default_rng(20261021)
    logits = (rng.standard_normal((12, A)) * 2.0).astype(np.float32)
    legal = np.zeros((12, A), dtype=bool)

    def put(b, actions, values):
        legal[b, actions] = True
        logits[b, actions] = np.asarray(values, dtype=np.float32)

    # 0: the top four equal, their mask words owned by waves 0, 1, 3 and 0 (thread = word % 256); six lower ones
    put(0, [5, 32 * 70 + 3, 32 * 200 + 1, 32 * 300], 2.5)
    put(0, [40, 4000, 8000, 9999, 11000, 11258], [1.0, 0.5, 1.0, -1.0, 0.25, 0.5])
    # 1: equal logits inside one word, below a single leader
    put(1, [32 * 100 + 1, 32 * 100 + 7, 32 * 100 + 20, 32 * 100 + 31], 1.75)
    put(1, [17, 6000, 6001, 9000, 10000], [3.0, 0.5, 0.5, -2.0, 0.0])
    # 2: six distinct leaders, then four equal logits for slots 6 and 7: two of them are cut
    put(2, [11, 2222, 3333, 4444, 5555, 6666], [6.0, 5.0, 4.0, 3.5, 3.0, 2.5])
    put(2, [9000, 31, 7777, 32 * 255 + 9], 2.0)
    put(2, [64, 65], [-1.0, -1.0])
    # 3: legal -inf (first and last action among them) beside nine finite logits, two of them equal
    put(3, [0, 777, 11258], -np.inf)
    put(3, [1, 300, 301, 2000, 4100, 6200, 8300, 10400, 11257], [0.5, 1.5, 1.5, -3.0, 2.0, 0.0, -0.5, 1.0, 0.25])
    # 4 (NAN_ROW): legal NaN and legal -inf beside nine finite logits
    put(4, [2, 5000, 11258], np.nan)
    put(4, [3, 9001], -np.inf)
    put(4, [4, 33, 600, 601, 2048, 4096, 8192, 10000, 11111], [1.0, 1.0, -0.5, 2.0, 0.75, -4.0, 3.0, 0.0, 1.0])
    # 5: fewer than 8 legal actions, a tie among them
    put(5, [9, 1000, 5000, 32 * 351, 11258], [0.5, -1.0, 0.5, 2.0, 0.5])
    # 6: the last bit of the last word alone
    put(6, [11258], -0.75)
    # 7: illegal actions carry the largest logits (and a NaN); the legal ones are the seeded background
    legal[7, rng.choice(A, size=40, replace=False)] = True
    illegal = np.flatnonzero(~legal[7])
    logits[7, illegal[::97]] = 50.0
    logits[7, illegal[5]] = np.nan
    # 8: every action legal, every logit equal
    put(8, np.arange(A), 0.25)
    # 9: the first and the last action equal at the top, a second tie across waves behind them
    put(9, [0, 11258], 4.0)
    put(9, [32 * 64, 32 * 128, 32 * 192, 32 * 256 + 31], 1.0)
    put(9, [500, 7000, 7001, 10500], [0.5, 0.0, -8.0, 2.0])
    # 10: logits far apart: most priors underflow
    put(10, [12, 345, 678, 901, 2345, 6789, 10111, 10112, 11200], [80.0, -100.0, 79.0, 0.0, -100.0, 40.0, -20.0, 80.0, -60.0])
    # 11: 300 legal actions of the seeded background
    legal[11, rng.choice(A, size=300, replace=False)] = True
    return logits, legal


def _order(logits, legal):
    """The third witness: finite legal logits by logit descending, then action ascending; -1 for unused slots.  With them the
    softmax over the legal logits that are not NaN, in float64."""
    actions = np.full((logits.shape[0], K), -1, dtype=np.int64)
    probs = np.zeros((logits.shape[0], K))
    for b in range(logits.shape[0]):
        z = logits[b].astype(np.float64)
        idx = np.flatnonzero(legal[b] & np.isfinite(z))
        top = idx[np.lexsort((idx, -z[idx]))][:K]
        weigh = np.flatnonzero(legal[b] & ~np.isnan(z))
        actions[b, :top.size] = top
        probs[b, :top.size] = np.exp(z[top] - z[weigh].max()) / np.exp(z[weigh] - z[weigh].max()).sum()
    return actions, probs


@functools.lru_cache(maxsize=None)
def _run(bf16: bool) -> dict:
    """The three launches over the 12 rows, once per dtype."""
    logits, legal = _rows()
    if bf16:
        logits = bf16_round(logits)
    B = logits.shape[0]
    st = _lib.stream_ptr(torch.device(DEV))
    lg = torch.from_numpy(logits).to(DEV)
    if bf16:
        lg = lg.to(torch.bfloat16)
    bits = torch.zeros(B, MASK_WORDS, dtype=torch.int32, device=DEV)
    _lib.call("ka_pack_mask_bits", torch.from_numpy(legal).to(DEV), bits, B, A, st)
    zeros64 = torch.zeros(B, dtype=torch.int64, device=DEV)
    model_of = torch.zeros(B, dtype=torch.int32, device=DEV)

    last = torch.zeros(B, insight_words(K), dtype=torch.int32, device=DEV)
    heat = torch.zeros(B, HEAT_WORDS, device=DEV)
    in_flags = torch.zeros(2, dtype=torch.int32, device=DEV)
    _lib.call("ka_policy_insight", lg, int(bf16), bits, MASK_WORDS, zeros64, None, None, None, 1, 1.0, K, last, heat, None, 0,
              None, in_flags, B, A, st)

    table = torch.from_numpy(lookahead_table(LookaheadControls(K), 1)).to(DEV)
    rec = torch.zeros(B, lookahead_words(K), dtype=torch.int32, device=DEV)
    _lib.call("ka_lookahead_fork", lg, int(bf16), bits, MASK_WORDS, zeros64, model_of, 1, table, None, None, None, 0, K, rec,
              None, None, None, None, None, None, B, A, st)

    greedy = torch.from_numpy(controls_table(SamplingControls.GREEDY, 1)).to(DEV)
    out = (torch.empty(B, dtype=torch.int64, device=DEV), torch.empty(B, device=DEV),
           torch.empty(B, dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV))
    _lib.call("ka_policy_sample_ctl", lg, int(bf16), bits, MASK_WORDS, zeros64[:1], model_of, 1, greedy, None, 0, *out, B, A, st)

    last, rec = last.cpu().numpy(), rec.cpu().numpy()
    want_actions, want_probs = _order(logits, legal)
    return {"legal": legal,
            "insight_actions": last[:, REC_TOP:REC_TOP + K], "insight_probs": last.view(np.float32)[:, REC_TOP + K:REC_TOP + 2 * K],
            "insight_nlegal": last[:, REC_NLEGAL], "insight_flags": in_flags.cpu().numpy(),
            "fork_actions": rec[:, REC_CAND:REC_CAND + K], "fork_priors": rec.view(np.float32)[:, REC_CAND + K:REC_CAND + 2 * K],
            "fork_ncand": rec[:, REC_NCAND], "greedy": out[0].cpu().numpy(), "ctl_nlegal": out[2].cpu().numpy(),
            "want_actions": want_actions, "want_probs": want_probs}


@DTYPES
def test_insight_and_fork_name_the_same_candidates(bf16):
    r = _run(bf16)
    assert r["insight_actions"].tolist() == r["fork_actions"].tolist()
    assert r["fork_ncand"].tolist() == (r["fork_actions"] >= 0).sum(axis=1).tolist()
    assert r["insight_nlegal"].tolist() == r["ctl_nlegal"].tolist() == r["legal"].sum(axis=1).tolist()


@DTYPES
def test_the_greedy_action_is_slot_zero(bf16):
    r = _run(bf16)
    assert r["greedy"].tolist() == r["insight_actions"][:, 0].tolist() == r["fork_actions"][:, 0].tolist()


@DTYPES
def test_the_numpy_order_is_the_third_witness(bf16):
    r = _run(bf16)
    assert r["insight_actions"].tolist() == r["want_actions"].tolist()
    assert r["fork_actions"].tolist() == r["want_actions"].tolist()
    if not bf16:                                               # what the rows were built to show, stated outright
        w = r["want_actions"]
        assert w[0].tolist() == [5, 32 * 70 + 3, 32 * 200 + 1, 32 * 300, 40, 8000, 4000, 11258]
        assert w[1, :5].tolist() == [17, 3201, 3207, 3220, 3231]
        assert w[2, 6:].tolist() == [31, 7777]
        assert w[5].tolist() == [32 * 351, 9, 5000, 11258, 1000, -1, -1, -1]
        assert w[6].tolist() == [11258] + [-1] * 7
        assert w[8].tolist() == list(range(8))
        assert w[9, :6].tolist() == [0, 11258, 10500, 32 * 64, 32 * 128, 32 * 192]
        assert (w[[3, 4, 7, 11]] >= 0).all()                   # their first 8 of the order are finite


@DTYPES
def test_the_forks_priors_are_the_insights_probabilities(bf16):
    r = _run(bf16)
    rows = [b for b in range(12) if b != NAN_ROW]
    np.testing.assert_allclose(r["fork_priors"][rows], r["insight_probs"][rows], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(r["fork_priors"], r["want_probs"], rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(r["insight_probs"][rows], r["want_probs"][rows], rtol=RTOL, atol=ATOL)
    # the row with a legal NaN: the insight's normaliser is NaN and it says so; an illegal NaN (row 7) raises nothing
    assert np.isnan(r["insight_probs"][NAN_ROW]).all() and r["insight_flags"].tolist() == [1, 0]
