"""Policy insight on the CPU: the float64 restatement behind `policy_insight` for CPU tensors against a numpy restatement
of the reference's showcase lines (runner.py:151-173, heatmap.py:40-49) written in the test helpers, `insight_dict` against
the restated runner and heatmap lines, the argument errors, and the header's declarations."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from keisei_amd import _lib
from keisei_amd.shogi_gym import MASK_WORDS
from keisei_amd.training import SelfPlayRollout, action_usi, insight_dict, policy_insight
from keisei_amd.training.policy_insight import HEAT_WORDS, InsightRecorder, history_fields, insight_words
from policy_insight_helpers import (A, DROP_SILVER, KNIGHT, PAWN_PUSH, SLOTS, as_numpy, bf16_round, build_heatmap, check_rows,
                                    crafted_rows, oracle_of, oracle_row, runner_candidates, seeded_rows, usi)

ROOT = Path(__file__).resolve().parent.parent


def _pack(legal: np.ndarray) -> torch.Tensor:
    bits = np.zeros((legal.shape[0], MASK_WORDS * 32), dtype=np.uint8)
    bits[:, :A] = legal
    words = np.packbits(bits.reshape(legal.shape[0], MASK_WORDS, 32), axis=2, bitorder="little").view(np.uint32)
    return torch.from_numpy(words.reshape(legal.shape[0], MASK_WORDS).view(np.int32).copy())


def _run(which, *, bf16=False, temperature=1.0, top_k=3, packed=False):
    logits, legal, actions, vlogits, players = crafted_rows() if which == "crafted" else seeded_rows()
    lg = torch.from_numpy(logits)
    if bf16:
        lg = lg.to(torch.bfloat16)
    lm = _pack(legal) if packed else torch.from_numpy(legal)
    return policy_insight(lg, lm, torch.from_numpy(actions), torch.from_numpy(vlogits), players=torch.from_numpy(players),
                          temperature=temperature, top_k=top_k)


@pytest.mark.parametrize("which", ["crafted", "seeded"])
@pytest.mark.parametrize("bf16,temperature,top_k,packed", [(False, 1.0, 3, False), (False, 0.5, 8, True), (True, 1.0, 1, True),
                                                             (True, 0.5, 3, False)])
def test_cpu_path_matches_the_oracle(which, bf16, temperature, top_k, packed):
    res = as_numpy(_run(which, bf16=bf16, temperature=temperature, top_k=top_k, packed=packed))
    check_rows(res, oracle_of(which, bf16, temperature), top_k, which)
    _, _, actions, _, players = crafted_rows() if which == "crafted" else seeded_rows()
    assert ((res["flags"] >> 1) & 1).tolist() == players.tolist()
    assert res["records"].shape == (len(actions), insight_words(top_k)) and not int(res["nan_flag"][0])
    assert res["records"][:, 1].tolist() == np.clip(actions, -1, A).tolist()


def test_crafted_rows_say_what_they_should():
    res = as_numpy(_run("crafted", top_k=8))
    assert res["chosen_probability"][0] == 1.0 and res["entropy"][0] == 0.0 and res["chosen_rank"][0] == 0
    assert res["top_actions"][0].tolist() == [PAWN_PUSH] + [-1] * 7 and res["top_probabilities"][0].tolist() == [1.0] + [0.0] * 7
    assert res["n_legal"].tolist() == [1, A, 9, 9, 10]
    assert np.count_nonzero(res["heat"][2]) == 5 and not res["heat"][2][81:].any()        # the drop's family runs over squares
    assert set(np.flatnonzero(res["heat"][3]).tolist()) == {0, 7, 64, 128, 129, 130, 131}  # the knight's runs over its slots
    assert res["top_actions"][4][:6].tolist() == [17, 4242, 9000, 11258, 10000, 5000]      # ties by lower action
    assert res["chosen_rank"][4] == 0                                                      # nothing is strictly greater
    assert np.unique(res["top_probabilities"][4][:4]).size == 1


def test_invalid_rows_and_the_nan_flag():
    logits, legal, actions, vlogits, _ = crafted_rows()
    lg, lm = torch.from_numpy(logits[:4].copy()), torch.from_numpy(legal[:4].copy())
    lm[1] = False                                                                          # no legal action
    res = as_numpy(policy_insight(lg, lm, torch.from_numpy(actions[:4]), torch.from_numpy(vlogits[:4]),
                                  model_of=torch.tensor([0, 0, -1, 1]), num_models=1, top_k=3))
    assert res["flags"].tolist() == [5, 0, 0, 0]
    assert not res["records"][1:].any() and not res["heat"][1:].any() and res["n_legal"][1] == 0
    assert insight_dict(res["records"][1], res["heat"][1]) is None
    assert history_fields(res["records"][2])["probability"] is None
    lg[0, PAWN_PUSH + 1] = float("nan")                                                    # an illegal logit: not flagged
    assert not int(policy_insight(lg[:1], lm[:1], torch.from_numpy(actions[:1])).nan_flag[0])
    lg[0, PAWN_PUSH] = float("nan")
    assert int(policy_insight(lg[:1], lm[:1], torch.from_numpy(actions[:1])).nan_flag[0])


def test_usi_of_both_colours():
    assert action_usi(PAWN_PUSH, 0) == "7g7f" and action_usi(PAWN_PUSH, 1) == "3c3d"
    assert action_usi(DROP_SILVER, 0) == "S*5e" and action_usi(DROP_SILVER, 1) == "S*5e"
    assert action_usi(40 * SLOTS + 132, 1) == "P*5e" and action_usi(0 * SLOTS + 138, 1) == "R*1i"
    assert action_usi(KNIGHT, 0) == "3g2e" and action_usi(KNIGHT, 1) == "7c8e"
    assert action_usi(70 * SLOTS + 64 + 7 * 8 + 5, 0) == "2h8b+" and action_usi(70 * SLOTS + 64 + 7 * 8 + 5, 1) == "8b2h+"
    assert action_usi(0, 0) == "?" and action_usi(A, 0) == "?"                             # off the board, outside the space
    rng = np.random.default_rng(3)
    for a in rng.integers(0, A, size=400).tolist():
        for colour in (0, 1):
            assert action_usi(a, colour) == (usi(a, colour) or "?"), (a, colour)


@pytest.mark.parametrize("row,temperature", [(2, 1.0), (3, 0.5), (4, 1.0), (0, 1.0)])
def test_insight_dict_restates_runner_and_heatmap(row, temperature):
    logits, legal, actions, vlogits, players = crafted_rows()
    res = as_numpy(_run("crafted", temperature=temperature, top_k=3))
    o = oracle_row(logits[row], legal[row], int(actions[row]), vlogits[row], temperature, 3)
    colour = int(players[row])
    d = insight_dict(res["records"][row], res["heat"][row])
    assert [(c["action"], c["usi"]) for c in d["top_candidates"]] == [(c["action"], c["usi"]) for c in runner_candidates(o, colour)]
    for c, want in zip(d["top_candidates"], runner_candidates(o, colour)):
        assert abs(c["probability"] - want["probability"]) <= 1.0001e-4                  # 4 places: at most one step apart
        assert c["probability"] == round(c["probability"], 4)
    legal_with_usi = [(int(a), usi(int(a), colour)) for a in np.flatnonzero(legal[row]) if usi(int(a), colour)]
    want = build_heatmap(usi(int(actions[row]), colour), legal_with_usi, {int(a): float(o["probs"][a]) for a in np.flatnonzero(legal[row])})
    assert set(d["move_heatmap"]) == set(want) and want
    for k, v in want.items():
        np.testing.assert_allclose(d["move_heatmap"][k], v, rtol=1e-4, atol=5e-5)
    assert d["move_usi"] == usi(int(actions[row]), colour) and d["action"] == int(actions[row])
    assert d["legal_moves"] == o["n_legal"] and d["chosen_rank"] == o["chosen_rank"]
    for key, okey in (("chosen_probability", "chosen_probability"), ("policy_entropy", "entropy"), ("win_probability", "win_probability")):
        np.testing.assert_allclose(d[key], o[okey], rtol=1e-4, atol=5e-5)
    h = history_fields(res["records"][row])
    assert h["top_candidates"] == d["top_candidates"] and h["rank"] == d["chosen_rank"] and h["probability"] == d["chosen_probability"]
    assert h["entropy"] == d["policy_entropy"] and h["win_probability"] == d["win_probability"]


def test_the_candidate_cut_and_the_rounding():
    """runner.py:172-173: a candidate at or below 0.001 is dropped, the others are rounded to 4 places."""
    legal = torch.zeros(1, A, dtype=torch.bool)
    idx = [PAWN_PUSH, PAWN_PUSH + 1, PAWN_PUSH + 2]
    legal[0, idx] = True
    lg = torch.zeros(1, A)
    lg[0, idx] = torch.tensor([0.0, -0.123456, -8.0])                  # p = 0.5308.., 0.4691.., 0.00017..
    r = policy_insight(lg, legal, torch.tensor([PAWN_PUSH]), top_k=3)
    p = np.exp(np.array([0.0, -0.123456, -8.0]))
    p /= p.sum()
    d = insight_dict(r.records[0], r.heat[0])
    assert d["top_candidates"] == [{"action": PAWN_PUSH, "probability": round(float(np.float32(p[0])), 4), "usi": "7g7f"},
                                   {"action": PAWN_PUSH + 1, "probability": round(float(np.float32(p[1])), 4), "usi": "7g7e"}]
    assert r.top_actions[0].tolist() == idx and 0 < float(r.top_probabilities[0, 2]) < 0.001
    assert d["win_probability"] == 0.0                                  # no value logits: 0, not NaN
    assert set(d["move_heatmap"]) == {"7g7f", "7g7e", "7g7d"}           # the cut is the candidates' alone


def test_argument_errors():
    lg, legal, act = torch.zeros(2, A), torch.ones(2, A, dtype=torch.bool), torch.zeros(2, dtype=torch.int64)
    for k in (0, 9, -1, 2.0, True):
        with pytest.raises(ValueError, match="top_k"):
            policy_insight(lg, legal, act, top_k=k)
    for t in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="temperature"):
            policy_insight(lg, legal, act, temperature=t)
    with pytest.raises(ValueError, match="spatial action space only"):
        policy_insight(torch.zeros(2, 13527), torch.ones(2, 13527, dtype=torch.bool), act)
    with pytest.raises(ValueError, match="legal must be bool"):
        policy_insight(lg, torch.ones(2, A), act)
    with pytest.raises(ValueError, match="expected 2 actions"):
        policy_insight(lg, legal, act[:1])
    with pytest.raises(ValueError, match="value_logits"):
        policy_insight(lg, legal, act, torch.zeros(2, 2))
    with pytest.raises(ValueError, match="32-bit words"):
        insight_dict(np.zeros(14, dtype=np.int64), np.zeros(HEAT_WORDS))
    with pytest.raises(ValueError, match="8 \\+ 2 top_k"):
        insight_dict(np.zeros(9, dtype=np.int32), np.zeros(HEAT_WORDS))
    with pytest.raises(ValueError, match="heat row"):
        insight_dict(np.array([1] + [0] * 13, dtype=np.int32), np.zeros(81))
    with pytest.raises(ValueError, match="spatial"):
        insight_dict(np.zeros(14, dtype=np.int32), np.zeros(HEAT_WORDS), "default")

    class Env:
        _amode, _hist, num_envs, device = 1, None, 2, torch.device("cpu")

    for k in (-1, 9, 2.5):
        with pytest.raises(ValueError, match="insight"):
            InsightRecorder(Env(), k)
    with pytest.raises(ValueError, match="insight_temperature"):
        InsightRecorder(Env(), 3, 0.0)
    import inspect
    for name in ("insight", "insight_temperature"):
        assert name in inspect.signature(SelfPlayRollout.__init__).parameters


def test_symbols_are_declared_and_bound():
    header = (ROOT / "include" / "keisei_amd.h").read_text()
    assert "policy insight" in header
    for name in ("ka_policy_insight", "ka_policy_insight_words"):
        assert re.search(rf"\bint {name}\(", header), name
        assert name in _lib.exported_symbols()
    if _lib.available():                                                # the layout the host decodes is the library's
        q = lambda which, k: _lib.query("ka_policy_insight_words", which, k)  # noqa: E731
        for k in (1, 3, 8):
            assert [q(i, k) for i in range(11)] == [insight_words(k), 0, 1, 2, 3, 4, 5, 6, 8, 8 + k, HEAT_WORDS]
        assert q(0, 0) == -1 and q(0, 9) == -1 and q(11, 3) == -1


def test_bf16_rounding_helper_matches_torch():
    x = np.random.default_rng(0).standard_normal(4096).astype(np.float32) * 5
    assert np.array_equal(bf16_round(x), torch.from_numpy(x).to(torch.bfloat16).float().numpy())
