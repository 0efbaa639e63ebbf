"""LeagueRollout without a GPU: the host restatement of the learner-vs-league rollout protocol against the reference's
own run (tests/golden/g13_league_rollout.npz, tools/make_league_golden.py), the numpy form of the re-draw function, and
the constructor's argument checks."""
from pathlib import Path

import numpy as np
import pytest
import torch

from keisei_amd.training import LeagueRollout, LeagueRolloutStats  # noqa: F401
from keisei_amd.training.league_rollout import (_league_host, cum_thresholds, draw_opponents, draw_sides, league_draw)
from keisei_amd.training.models.se_resnet import SEResNetModel, SEResNetParams
from keisei_amd.training.value_adapter import ScalarValueAdapter
from oracle import keisei_oracle as orc

GOLDEN = Path(__file__).resolve().parent / "golden" / "g13_league_rollout.npz"
COLUMNS = ("observations", "actions", "log_probs", "values", "rewards", "dones", "terminated", "legal_masks",
           "value_categories", "score_targets", "env_ids", "next_value_override")


def _fixture():
    z = np.load(GOLDEN)
    T = z["stream_rewards"].shape[0]
    keys = [k[len("stream_"):] for k in z.files if k.startswith("stream_")]
    records = [{k: z["stream_" + k][t] for k in keys} for t in range(T)]
    return z, records


def _run_host(z, records, **over):
    kw = dict(num_envs=int(z["side0"].shape[0]), obs_shape=tuple(int(v) for v in z["obs_shape"]),
              action_space=int(z["action_space"]), opponent_ids=[int(v) for v in z["opponent_ids"]], seed=int(z["draw_seed"]),
              cum=z["cum"], color_randomization=True, score_norm=float(z["score_norm"]), side=z["side0"], opp=z["opp0"])
    kw.update(over)
    return _league_host(records, **kw)


def test_host_restatement_equals_the_reference_run():
    z, records = _fixture()
    cols, stats = _run_host(z, records)
    assert cols["size"] == int(z["size"]) == stats["adds"]
    for key in COLUMNS:
        want, got = z["col_" + key], cols[key].numpy()
        assert got.dtype == want.dtype and got.shape == want.shape, key
        assert np.array_equal(got, want, equal_nan=key == "next_value_override"), key
    ov = z["col_next_value_override"]
    assert np.isfinite(ov).sum() == int(z["tally_truncation_overrides"]) > 0 and np.isnan(ov).any()
    for k in ("wins", "losses", "draws", "black_wins", "white_wins", "terminated", "truncated", "truncation_overrides"):
        assert stats[k] == int(z["tally_" + k]), k
    assert stats["rows"] == z["col_actions"].shape[0] and stats["plies"] == len(records)
    want = {int(o): [int(v) for v in r] for o, r in zip(z["opponent_ids"], z["opponent_results"])}
    assert stats["opponent_results"] == want
    assert sum(sum(r) for r in want.values()) == stats["terminated"]


def test_fixture_reaches_every_branch_of_the_protocol():
    z, records = _fixture()
    d, t = z["col_dones"], z["col_terminated"]
    assert (d & t).any() and (d & ~t).any() and (~d).any()
    assert (z["col_value_categories"] == 1).any()                         # a draw
    assert set(np.unique(z["col_value_categories"])) == {-1, 0, 1, 2}
    trace = []
    _run_host(z, records, trace=trace)
    sides = np.stack([z["side0"], *(tr["side"] for tr in trace[:-1])])   # the side of every ply's game
    moved = z["stream_pre_players"] == sides
    assert (sides == 0).any() and (sides == 1).any()
    assert (~moved).all(axis=1).any() and moved.all(axis=1).any()         # a ply without a learner move, one without an opponent move
    done = z["stream_terminated"] | z["stream_truncated"]
    assert (done[1:] & done[:-1]).any()                                   # an env done on consecutive plies
    assert (moved & done).any() and (~moved & done).any()                 # either mover ends a game
    trunc = z["stream_truncated"] & ~z["stream_terminated"]
    assert (moved & trunc).any() and (~moved & trunc).any()
    assert trace[-1]["valid"].any()                                       # a pending row left for the flush


def test_host_restatement_sees_a_changed_rule():
    """The fixture has the teeth the seeded errors need: a restatement that forgets the opponent's negation, or that is
    handed other draws, does not reproduce the reference's columns."""
    z, records = _fixture()
    flipped = [dict(r, pre_players=1 - r["pre_players"]) for r in records]
    cols, _ = _run_host(z, flipped, side=1 - z["side0"], color_randomization=False)
    assert cols["rewards"].shape != z["col_rewards"].shape or not np.array_equal(cols["rewards"].numpy(), z["col_rewards"])
    cols, stats = _run_host(z, records, seed=int(z["draw_seed"]) + 1)
    want = {int(o): [int(v) for v in r] for o, r in zip(z["opponent_ids"], z["opponent_results"])}
    assert stats["opponent_results"] != want


# ------------------------------------------------------------------ draws
def test_draws_lie_in_range_and_are_stateless():
    cum = cum_thresholds([1.0, 0.0, 2.5, 1.5, 0.0], 5)
    env, n = np.arange(4096) % 512, np.arange(4096) // 512
    k = draw_opponents(99, env, n, cum)
    s = draw_sides(99, env, n)
    assert k.min() >= 0 and k.max() < 5 and set(np.unique(s)) <= {0, 1}
    assert not np.isin(k, (1, 4)).any()                                   # an opponent without weight is never drawn
    assert np.array_equal(k[1000:1010], draw_opponents(99, env[1000:1010], n[1000:1010], cum))
    assert int(league_draw(99, 7, 3, 5)) == int(league_draw(99, 7, np.array([3]), np.array([5]))[0])
    assert not np.array_equal(k, draw_opponents(100, env, n, cum))
    one = draw_opponents(5, env, n, cum_thresholds(None, 1))
    assert (one == 0).all()


@pytest.mark.parametrize("weights", [None, [1.0, 3.0, 2.0, 2.0], [5.0, 0.0, 1.0, 0.5]])
def test_draw_frequencies_follow_the_weights(weights):
    n_draws = 100_000
    K = 4
    cum = cum_thresholds(weights, K)
    env, n = np.arange(n_draws) % 512, np.arange(n_draws) // 512
    k = draw_opponents(0xC0FFEE, env, n, cum)
    p = np.full(K, 1 / K) if weights is None else np.asarray(weights) / np.sum(weights)
    counts = np.bincount(k, minlength=K)
    sigma = np.sqrt(n_draws * p * (1 - p))
    assert (np.abs(counts - n_draws * p) <= 5 * sigma + 1e-9).all(), (counts, n_draws * p, sigma)
    ones = int(draw_sides(0xC0FFEE, env, n).sum())
    assert abs(ones - n_draws / 2) <= 5 * np.sqrt(n_draws / 4)


def test_thresholds_reject_bad_weights():
    for bad in ([1.0, 2.0], [1.0, -1.0, 1.0], [0.0, 0.0, 0.0], [1.0, float("nan"), 1.0]):
        with pytest.raises(ValueError, match="opponent_weights"):
            cum_thresholds(bad, 3)
    cum = cum_thresholds([1, 1, 2], 3)
    assert cum.dtype == np.uint32 and list(cum) == [1 << 29, 1 << 30, 1 << 31]


# ------------------------------------------------------------------ constructor
SHAPE = orc.NetShape(2, 32, 8, 16, 8, 32, 16)


def _model(shape=SHAPE):
    return SEResNetModel(SEResNetParams(**shape.__dict__)).eval()


def test_constructor_and_argument_errors():
    a, b = _model(), _model()
    ok = dict(num_envs=8, max_ply=40, sync_every=8)
    with pytest.raises(ValueError, match="at least one opponent"):
        LeagueRollout(a, [], [], **ok)
    with pytest.raises(ValueError, match="opponent_ids"):
        LeagueRollout(a, [b], [1, 2], **ok)
    with pytest.raises(ValueError, match="opponent_ids"):
        LeagueRollout(a, [b, b], [3, 3], **ok)
    with pytest.raises(ValueError, match="sync_every .* must not exceed max_ply"):
        LeagueRollout(a, [b], [1], num_envs=8, max_ply=4, sync_every=8)
    with pytest.raises(ValueError, match="even sync_every"):
        LeagueRollout(a, [b], [1], num_envs=8, max_ply=40, sync_every=7, graph=True)
    with pytest.raises(ValueError, match="record=True runs without a graph"):
        LeagueRollout(a, [b], [1], record=True, **ok)
    with pytest.raises(ValueError, match="num_envs"):
        LeagueRollout(a, [b], [1], num_envs=0, max_ply=40, sync_every=8)
    with pytest.raises(ValueError, match="max_ply"):
        LeagueRollout(a, [b], [1], num_envs=8, max_ply=70000, sync_every=8)
    with pytest.raises(ValueError, match="score_norm"):
        LeagueRollout(a, [b], [1], score_norm=0.0, **ok)
    with pytest.raises(ValueError, match="MultiHeadValueAdapter"):
        LeagueRollout(a, [b], [1], value_adapter=ScalarValueAdapter(), **ok)
    with pytest.raises(ValueError, match="opponent_weights"):
        LeagueRollout(a, [b], [1], opponent_weights=[1.0, 2.0], **ok)
    wide = _model(orc.NetShape(2, 64, 8, 16, 8, 32, 16))
    with pytest.raises(ValueError, match="split_merge_step"):                # a shape mismatch names the path to use instead
        LeagueRollout(a, [b, wide], [1, 2], **ok)
    with pytest.raises(ValueError, match="split_merge_step"):                # CPU models: there is no CPU rollout
        LeagueRollout(a, [b], [1], **ok)
