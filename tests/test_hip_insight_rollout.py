"""The policy insight inside the device rollouts' ply: SelfPlayRollout, LeagueRollout and MatchArena built with
`insight=3`.  The logits of the recorded plies are recomputed with the group forward on the recorded observations and the
figures `spectator_data()` hands out are held to the float64 restatement of the reference's showcase lines
(policy_insight_helpers.oracle_row).  The smallest tower the device group covers (2 x 128), 8 envs and max_ply 6: games
end and histories clear inside the test."""
import gc
import json

import numpy as np
import pytest
import torch

from keisei_amd.shogi_gym import ACTION_SPACE
from keisei_amd.training import LeagueRollout, MatchArena, SelfPlayRollout
from keisei_amd.training.katago_ppo import KataGoRolloutBuffer
from keisei_amd.training.model_group import SEResNetGroup
from keisei_amd.training.models.se_resnet import SEResNetModel, SEResNetParams
from oracle import keisei_oracle as orc
from policy_insight_helpers import ATOL, RTOL, oracle_row, runner_candidates, usi

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPE = orc.NetShape(2, 128, 8, 64, 16, 128, 64)                 # the smallest tower the device group covers (128 channels)
OBS = (50, 9, 9)
N, MAX_PLY, TOP_K = 8, 6, 3
NEW_KEYS = {"probability", "rank", "entropy", "win_probability", "top_candidates"}
_MODELS = {}


@pytest.fixture(autouse=True)
def _release_device_objects():
    """(see tests/test_hip_selfplay_rollout.py: rollout objects own captured graphs and pinned buffers)"""
    yield
    gc.collect()
    torch.cuda.synchronize()
    gc.collect()


def _model(salt=7):
    if salt not in _MODELS:
        m = SEResNetModel(SEResNetParams(**SHAPE.__dict__))
        m.load_state_dict(orc.init_like_state_dict(SHAPE, salt=salt), strict=True)
        _MODELS[salt] = m.to(DEV).eval()
    return _MODELS[salt]


def _unpack(bits) -> np.ndarray:
    words = np.asarray(bits).astype(np.int32).view(np.uint32)
    j = np.arange(ACTION_SPACE)
    return ((words[:, j >> 5] >> (j & 31).astype(np.uint32)) & 1).astype(bool)


def _oracle_of_ply(roll, rec, temperature=1.0):
    """The oracle of every env for one recorded ply: the group forward on the recorded observations, then float64."""
    n = rec["obs"].shape[0]
    model_of = torch.as_tensor(np.asarray(rec["model_of"]) if "model_of" in rec else np.zeros(n), dtype=torch.int32)
    out = roll.group.forward(rec["obs"].to(DEV), model_of.to(DEV))
    logits = out.policy_logits.reshape(n, ACTION_SPACE).double().cpu().numpy()
    vlogits = out.value_logits.double().cpu().numpy()
    legal = _unpack(rec["mask_bits"])
    actions = np.asarray(rec["actions"])
    return [oracle_row(logits[e], legal[e], int(actions[e]), vlogits[e], temperature, TOP_K) for e in range(n)]


def _close(got, want, what):
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, err_msg=what)


def _check_candidates(got, o, colour, what):
    want = runner_candidates(o, colour)
    assert [(c["action"], c["usi"]) for c in got] == [(c["action"], c["usi"]) for c in want], what
    for c, w in zip(got, want):
        assert abs(c["probability"] - w["probability"]) <= 1.0001e-4, what      # 4 places: at most one step apart


def _check_against_the_records(roll, data, temperature=1.0):
    """`insight` of every env against the last recorded ply; every history entry against the ply it was played in."""
    records = roll.record
    oracles = {}
    for e, d in enumerate(data):
        rec = records[-1]
        o = oracles.setdefault(len(records) - 1, _oracle_of_ply(roll, rec, temperature))[e]
        colour, ins = int(np.asarray(rec["pre_players"])[e]), d["insight"]
        what = f"env {e}"
        assert ins is not None and o["legal_action"], what
        assert ins["action"] == int(np.asarray(rec["actions"])[e]) and ins["move_usi"] == usi(ins["action"], colour), what
        assert ins["legal_moves"] == o["n_legal"] == int(np.asarray(rec["n_legal"])[e]) and ins["chosen_rank"] == o["chosen_rank"], what
        _close(ins["chosen_probability"], o["chosen_probability"], what)
        _close(ins["chosen_probability"], np.exp(float(np.asarray(rec["log_probs"])[e])), what + ": the sampler's own log-prob")
        _close(ins["policy_entropy"], o["entropy"], what)
        _close(ins["win_probability"], o["win_probability"], what)
        _check_candidates(ins["top_candidates"], o, colour, what)
        legal = np.flatnonzero(_unpack(rec["mask_bits"])[e])
        prefix = ins["move_usi"][:2]
        family = {usi(int(a), colour): float(o["probs"][a]) for a in legal if usi(int(a), colour)[:2] == prefix and o["probs"][a] > 0}
        assert set(ins["move_heatmap"]) == set(family) and ins["move_usi"] in family, what
        for k, v in family.items():
            _close(ins["move_heatmap"][k], v, f"{what} heat {k}")
        hist = d["move_history"]
        assert len(hist) == d["ply"], what
        for i, entry in enumerate(hist):
            t = len(records) - len(hist) + i
            rec_t = records[t]
            o_t = oracles.setdefault(t, _oracle_of_ply(roll, rec_t, temperature))[e]
            what_t = f"env {e} move {i}"
            assert NEW_KEYS <= set(entry) and entry["action"] == int(np.asarray(rec_t["actions"])[e]), what_t
            assert entry["rank"] == o_t["chosen_rank"], what_t
            _close(entry["probability"], o_t["chosen_probability"], what_t)
            _close(entry["entropy"], o_t["entropy"], what_t)
            _close(entry["win_probability"], o_t["win_probability"], what_t)
            _check_candidates(entry["top_candidates"], o_t, int(np.asarray(rec_t["pre_players"])[e]), what_t)
        if hist:
            assert hist[-1]["probability"] == ins["chosen_probability"] and hist[-1]["top_candidates"] == ins["top_candidates"], what


def _selfplay(graph, sync_every, plies=8, **kw):
    roll = SelfPlayRollout(_model(), num_envs=N, max_ply=MAX_PLY, graph=graph, sync_every=sync_every, seed=5,
                           move_history=True, **kw)
    roll.collect(KataGoRolloutBuffer(N, OBS, ACTION_SPACE, device=DEV), plies)
    return roll, roll.spectator_data()


def test_selfplay_insight_matches_the_oracle_on_the_recorded_plies():
    roll, data = _selfplay(False, 2, insight=TOP_K, record=True)
    assert len(roll.record) == 8 and sum(len(d["move_history"]) for d in data) > 0
    assert all(d["ply"] <= 8 - MAX_PLY for d in data)          # every game was truncated at ply 6: the histories were cleared
    _check_against_the_records(roll, data)
    assert roll.spectator_data([5, 1]) == [data[5], data[1]]
    json.dumps(data)


def test_selfplay_insight_at_another_temperature():
    roll, data = _selfplay(False, 2, plies=4, insight=TOP_K, insight_temperature=0.5, record=True)
    for e, (d, o) in enumerate(zip(data, _oracle_of_ply(roll, roll.record[-1], 0.5))):
        _close(d["insight"]["chosen_probability"], o["chosen_probability"], f"env {e}")
        _close(d["insight"]["policy_entropy"], o["entropy"], f"env {e}")
        assert len(d["move_history"]) == d["ply"] == 4


def test_captured_and_eager_plies_give_identical_insight():
    (_, a), (_, b) = _selfplay(True, 4, insight=TOP_K), _selfplay(False, 2, insight=TOP_K)
    assert a == b
    assert all(d["insight"] is not None and NEW_KEYS <= set(m) for d in a for m in d["move_history"])
    assert all(len(d["move_history"]) == d["ply"] for d in a)


def test_before_the_first_move_there_is_no_insight():
    roll, data = _selfplay(False, 2, plies=2, insight=TOP_K)
    assert all(d["insight"] is not None for d in data)
    roll.reset()
    fresh = roll.spectator_data()
    assert all(d["insight"] is None and d["move_history"] == [] for d in fresh)


def test_insight_off_changes_no_dict_and_allocates_nothing():
    roll, data = _selfplay(True, 4)
    assert roll.insight is None
    assert all("insight" not in d for d in data)
    assert all(set(m) == {"action", "notation", "usi"} for d in data for m in d["move_history"])
    assert sum(len(d["move_history"]) for d in data) > 0
    for bad in (-1, 9):
        with pytest.raises(ValueError, match="insight"):
            SelfPlayRollout(_model(), num_envs=N, max_ply=MAX_PLY, graph=False, sync_every=2, insight=bad)
    with pytest.raises(ValueError, match="insight_temperature"):
        SelfPlayRollout(_model(), num_envs=N, max_ply=MAX_PLY, graph=False, sync_every=2, insight=3, insight_temperature=0.0)


def test_league_rollout_insight_matches_the_oracle():
    league = LeagueRollout(_model(1), [_model(2)], [10], num_envs=N, max_ply=MAX_PLY, graph=False, sync_every=2, seed=3,
                           move_history=True, insight=TOP_K, record=True)
    league.collect(KataGoRolloutBuffer(N, OBS, ACTION_SPACE, device=DEV), 8)
    data = league.spectator_data()
    assert {int(m) for rec in league.record for m in np.asarray(rec["model_of"])} == {0, 1}      # both models moved
    _check_against_the_records(league, data)
    captured = LeagueRollout(_model(1), [_model(2)], [10], num_envs=N, max_ply=MAX_PLY, graph=True, sync_every=4, seed=3,
                             move_history=True, insight=TOP_K)
    captured.collect(KataGoRolloutBuffer(N, OBS, ACTION_SPACE, device=DEV), 8)
    assert captured.spectator_data() == data


def test_an_idle_arena_slot_reports_no_insight():
    arena = MatchArena(SEResNetGroup([_model(1), _model(2)]), num_envs=N, envs_per_match=4, max_ply=MAX_PLY, sync_every=4, seed=3,
                       graph=False, move_history=True, insight=TOP_K, record=True)
    arena.run_round([(0, 1)], games_per_match=4, max_ply=2)     # the ply ceiling ends the pairing after 4 plies, mid-game
    data = arena.spectator_data()
    assert len(arena.record) == 4 and all(d["ply"] == 4 and len(d["move_history"]) == 4 for d in data)
    rec = arena.record[-1]
    oracle = _oracle_of_ply(arena, rec)
    for e in range(4):                                          # the seated slot
        ins, colour = data[e]["insight"], int(np.asarray(rec["pre_players"])[e])
        assert ins is not None and ins["action"] == int(np.asarray(rec["actions"])[e])
        assert ins["chosen_rank"] == oracle[e]["chosen_rank"] and ins["legal_moves"] == oracle[e]["n_legal"]
        _close(ins["chosen_probability"], oracle[e]["chosen_probability"], f"env {e}")
        _close(ins["win_probability"], oracle[e]["win_probability"], f"env {e}")     # the arena keeps the value output for this
        _check_candidates(ins["top_candidates"], oracle[e], colour, f"env {e}")
        assert all(m["probability"] is not None and m["top_candidates"] for m in data[e]["move_history"])
    for e in range(4, 8):                                       # the idle slot: its envs move (first legal action), nobody chose
        assert data[e]["insight"] is None
        assert all(m["probability"] is None and m["rank"] is None and m["top_candidates"] == [] for m in data[e]["move_history"])
    plain = MatchArena(SEResNetGroup([_model(1), _model(2)]), num_envs=N, envs_per_match=4, max_ply=MAX_PLY, sync_every=4, seed=3,
                       graph=True, move_history=True)
    plain.run_round([(0, 1)], games_per_match=4, max_ply=2)
    assert all("insight" not in d and all(set(m) == {"action", "notation", "usi"} for m in d["move_history"])
               for d in plain.spectator_data())
