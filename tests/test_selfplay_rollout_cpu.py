"""SelfPlayRollout without a GPU: the host restatement of the self-play (no-opponent) rollout branch against the reference's
own run (tests/golden/g14_selfplay_rollout.npz, tools/make_selfplay_golden.py), the branches the fixture reaches, the
restatement's teeth, and the constructor's argument checks."""
from pathlib import Path

import numpy as np
import pytest
import torch

from keisei_amd import _lib
from keisei_amd.training import SelfPlayRollout, SelfPlayStats  # noqa: F401
from keisei_amd.training import selfplay_rollout as spr
from keisei_amd.training.katago_loop import _compute_value_cats
from keisei_amd.training.katago_ppo import KataGoRolloutBuffer
from keisei_amd.training.models.se_resnet import SEResNetModel, SEResNetParams
from keisei_amd.training.value_adapter import ScalarValueAdapter
from oracle import keisei_oracle as orc

GOLDEN = Path(__file__).resolve().parent / "golden" / "g14_selfplay_rollout.npz"
COLUMNS = ("observations", "actions", "log_probs", "values", "rewards", "dones", "terminated", "legal_masks",
           "value_categories", "score_targets", "next_value_override")
TALLIES = ("wins", "losses", "draws", "black_wins", "white_wins", "terminated", "truncated", "truncation_overrides")


def _fixture():
    z = np.load(GOLDEN)
    T = z["stream_rewards"].shape[0]
    keys = [k[len("stream_"):] for k in z.files if k.startswith("stream_")]
    records = [{k: z["stream_" + k][t] for k in keys} for t in range(T)]
    return z, records


def _run_host(z, records, **over):
    kw = dict(num_envs=int(z["stream_rewards"].shape[1]), obs_shape=tuple(int(v) for v in z["obs_shape"]),
              action_space=int(z["action_space"]), score_norm=float(z["score_norm"]), final_values=z["final_values"])
    kw.update(over)
    return spr._selfplay_host(records, **kw)


def _differs(cols, z):
    return any(not np.array_equal(cols[k].numpy(), z["col_" + k], equal_nan=True) for k in COLUMNS)


def test_host_restatement_equals_the_reference_run():
    z, records = _fixture()
    cols, stats = _run_host(z, records)
    assert cols["size"] == int(z["size"]) == len(records)
    assert "env_ids" not in cols and "col_env_ids" not in z.files
    for key in COLUMNS:
        want, got = z["col_" + key], cols[key].numpy()
        assert got.dtype == want.dtype and got.shape == want.shape, key
        assert np.array_equal(got, want, equal_nan=key == "next_value_override"), key
    for k in TALLIES:
        assert stats[k] == int(z["tally_" + k]), k
    assert stats["rows"] == z["col_actions"].shape[0] == len(records) * z["stream_rewards"].shape[1]
    assert stats["plies"] == len(records)
    assert np.array_equal(cols["next_values"].numpy(), z["next_values"])
    assert np.array_equal(z["next_values"], -z["final_values"])
    assert not _differs(cols, z)


def test_fixture_reaches_every_branch_of_the_protocol():
    z, _ = _fixture()
    tm, tr, r, pre = z["stream_terminated"], z["stream_truncated"], z["stream_rewards"], z["stream_pre_players"]
    done, trunc = tm | tr, tr & ~tm
    assert (tm & (r > 0) & (pre == 0)).any(), "a mover's win as black"
    assert (tm & (r > 0) & (pre == 1)).any(), "a mover's win as white"
    assert (tm & (r < 0)).any(), "a mover's loss"
    assert (tm & (r == 0)).any(), "a draw"
    assert trunc.any(), "a truncation without termination"
    assert (done[1:] & done[:-1]).any(), "an env done on two consecutive plies"
    assert trunc[0].any() and trunc[-1].any(), "a truncation on the first and on the last ply"
    assert (tm[:-1] & ~done[1:]).any(), "a terminated row directly in front of a non-terminal one"
    assert (tm & tr).any(), "a game decided on the ply that would have truncated it"
    # that pair makes the alternating fill both skip and act; the truncated rows carry the override they were given
    T, E = tm.shape
    ov = z["col_next_value_override"].reshape(T, E)
    vals = z["col_values"].reshape(T, E)
    assert np.isnan(ov[:-1][tm[:-1]]).all() and np.isfinite(ov[:-1][~tm[:-1]]).all()
    assert np.array_equal(ov[trunc], -z["stream_term_values"][trunc])
    open_ = ~done[:-1]
    assert open_.any() and np.array_equal(ov[:-1][open_], -vals[1:][open_])
    assert set(np.unique(z["col_value_categories"])) == {-1, 0, 1, 2}
    last = ov[-1]
    assert np.isnan(last[~trunc[-1]]).all()                              # the last ply bootstraps from next_values


def test_host_restatement_sees_a_changed_rule(monkeypatch):
    """A restatement with one rule flipped does not reproduce the reference's columns."""
    z, records = _fixture()
    with monkeypatch.context() as m:                                      # the truncation test without its ~terminated
        m.setattr(spr, "_truncated_only", lambda terminated, truncated: truncated)
        cols, _ = _run_host(z, records)
        assert _differs(cols, z)
    with monkeypatch.context() as m:                                      # the override without its sign
        m.setattr(spr, "_override_of", lambda v: v)
        cols, _ = _run_host(z, records)
        assert _differs(cols, z)
        assert all(np.array_equal(cols[k].numpy(), z["col_" + k]) for k in COLUMNS[:-1])
    with monkeypatch.context() as m:                                      # labels from the negated reward
        m.setattr(spr, "_compute_value_cats", lambda r, t, d: _compute_value_cats(-r, t, d))
        cols, _ = _run_host(z, records)
        assert not np.array_equal(cols["value_categories"].numpy(), z["col_value_categories"])
    _, stats = _run_host(z, [dict(r, pre_players=1 - r["pre_players"]) for r in records])
    assert (stats["black_wins"], stats["white_wins"]) == (int(z["tally_white_wins"]), int(z["tally_black_wins"]))
    cols, _ = _run_host(z, records)                                       # and, restored, it does again
    assert not _differs(cols, z)


def test_one_host_run_against_two_halves():
    """The fill at the end of every call only fills NaN cells, so going on from a prior buffer gives the same columns."""
    z, records = _fixture()
    whole, _ = _run_host(z, records)
    kw = dict(num_envs=4, obs_shape=tuple(int(v) for v in z["obs_shape"]), action_space=int(z["action_space"]),
              score_norm=float(z["score_norm"]))
    prior = KataGoRolloutBuffer(4, kw["obs_shape"], kw["action_space"])
    spr._selfplay_host(records[:11], prior=prior, **kw)
    halves, _ = spr._selfplay_host(records[11:], prior=prior, **kw)
    for key in COLUMNS:
        assert np.array_equal(whole[key].numpy(), halves[key].numpy(), equal_nan=True), key
    assert halves["size"] == whole["size"]


# ------------------------------------------------------------------ constructor
SHAPE = orc.NetShape(2, 32, 8, 16, 8, 32, 16)


def _model(shape=SHAPE):
    return SEResNetModel(SEResNetParams(**shape.__dict__)).eval()


def test_constructor_and_argument_errors():
    a = _model()
    ok = dict(num_envs=8, max_ply=40, sync_every=8)
    with pytest.raises(ValueError, match="sync_every .* must not exceed max_ply"):
        SelfPlayRollout(a, num_envs=8, max_ply=4, sync_every=8)
    with pytest.raises(ValueError, match="even sync_every"):
        SelfPlayRollout(a, num_envs=8, max_ply=40, sync_every=7, graph=True)
    with pytest.raises(ValueError, match="record=True runs without a graph"):
        SelfPlayRollout(a, record=True, **ok)
    with pytest.raises(ValueError, match="num_envs"):
        SelfPlayRollout(a, num_envs=0, max_ply=40, sync_every=8)
    with pytest.raises(ValueError, match="max_ply"):
        SelfPlayRollout(a, num_envs=8, max_ply=70000, sync_every=8)
    with pytest.raises(ValueError, match="sync_every must be at least 1"):
        SelfPlayRollout(a, num_envs=8, max_ply=40, sync_every=0)
    with pytest.raises(ValueError, match="score_norm"):
        SelfPlayRollout(a, score_norm=0.0, **ok)
    with pytest.raises(ValueError, match="MultiHeadValueAdapter"):
        SelfPlayRollout(a, value_adapter=ScalarValueAdapter(), **ok)
    with pytest.raises(ValueError, match="select_actions' loop"):           # a CPU model: there is no CPU rollout
        SelfPlayRollout(a, **ok)
    with pytest.raises(ValueError, match="select_actions' loop"):           # not an SEResNetModel
        SelfPlayRollout(torch.nn.Linear(2, 2), **ok)
    assert SelfPlayStats().host_syncs == 0


def test_library_binding_names_the_new_entry_points():
    names = _lib.exported_symbols()
    assert {"ka_selfplay_step", "ka_selfplay_state_words", "ka_selfplay_layout"} <= set(names)
    header = (Path(__file__).resolve().parent.parent / "include" / "keisei_amd.h").read_text()
    for n in ("ka_selfplay_step", "ka_selfplay_state_words", "ka_selfplay_layout"):
        assert f"int {n}(" in header, n


def test_reserve_refuses_the_host_store_whatever_the_layout():
    buf = KataGoRolloutBuffer(4, (2, 3, 3), 40, device="cpu")
    with pytest.raises(ValueError, match="device-resident"):
        buf.reserve(8, env_ids=False)
    assert buf._has_env_ids is False and "env_ids" not in buf._storage
