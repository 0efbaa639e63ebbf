"""Sampling controls in the owners' plies: MatchArena(sampling=), set_sampling, LeagueRollout(opponent_sampling=)."""
import gc

import numpy as np
import pytest
import torch

from keisei_amd import _lib
from keisei_amd.shogi_gym import ACTION_SPACE, MASK_WORDS
from keisei_amd.training import LeagueRollout, MatchArena, SamplingControls, controls_table, sample_controlled
from keisei_amd.training.katago_ppo import KataGoRolloutBuffer
from keisei_amd.training.league_rollout import _league_host
from keisei_amd.training.model_group import SEResNetGroup
from keisei_amd.training.models.se_resnet import SEResNetModel, SEResNetParams
from keisei_amd.training.value_adapter import MultiHeadValueAdapter
from oracle import keisei_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPE = orc.NetShape(2, 128, 8, 64, 16, 128, 64)
MAX_PLY = 40
N, PER = 16, 8
OBS = (50, 9, 9)
PAIRINGS = [(0, 1), (1, 0), (1, 1)]                          # more pairings than slots, one model against itself
GREEDY, NEUTRAL = SamplingControls.GREEDY, SamplingControls.NEUTRAL
_MODELS = []
_GROUP = {}


@pytest.fixture(autouse=True)
def _release_device_objects():
    """Arenas and rollouts own captured graphs and pinned buffers: collect them with the device idle, not inside a later
    test's capture (tests/test_hip_league_rollout.py)."""
    yield
    gc.collect()
    torch.cuda.synchronize()
    gc.collect()


def _models(n):
    while len(_MODELS) < n:
        m = SEResNetModel(SEResNetParams(**SHAPE.__dict__))
        m.load_state_dict(orc.init_like_state_dict(SHAPE, salt=31 * len(_MODELS) + 7), strict=True)
        _MODELS.append(m.to(DEV).eval())
    return _MODELS[:n]


def _group():
    if 2 not in _GROUP:
        _GROUP[2] = SEResNetGroup(_models(2))
    return _GROUP[2]


def _stream():
    return _lib.stream_ptr(torch.device(DEV))


def _masks(bits):
    B = bits.shape[0]
    masks = torch.empty(B, ACTION_SPACE, dtype=torch.bool, device=DEV)
    _lib.call("ka_unpack_mask_bits", bits, None, masks, B, ACTION_SPACE, _stream())
    return masks


def _key(results):
    return [(r.a, r.b, r.a_wins, r.b_wins, r.draws, r.plies, r.partial) for r in results]


def _own_games(results):
    """per pairing, the move lists of its finished games that the pairing played from the first ply on"""
    out = []
    for r in results:
        games = [g for g in r.recorded_games if g.finished and not g.carried]
        out.append([tuple(int(a) for a in g.actions) for g in games])
    return out


def _all_identical(results, least=2):
    """(16 games on 8 envs are at least two waves: the second one starts under the pairing that finishes it)"""
    per = _own_games(results)
    assert all(len(games) >= least for games in per), [len(g) for g in per]
    return all(len(set(games)) == 1 for games in per)


# ------------------------------------------------------------------ the arena's ply, replayed
def test_recorded_arena_plies_replay_through_sample_controlled():
    grp = _group()
    ctl = [GREEDY, NEUTRAL]
    arena = MatchArena(grp, N, PER, MAX_PLY, sync_every=2, graph=False, seed=11, record=True, sampling=ctl)
    arena.run_round(PAIRINGS, games_per_match=8)
    recs = arena.record
    assert len(recs) >= 20
    greedy_rows = neutral_rows = late = 0
    for t, rec in enumerate(recs):
        mo = rec["model_of"].to(DEV)
        bits = rec["mask_bits"].to(DEV)
        logits = grp.forward(rec["obs"].to(DEV), mo, check=False).policy_logits.reshape(N, ACTION_SPACE).contiguous()
        got = sample_controlled(logits, bits, rec["seed"], controls=ctl, model_of=mo, plies=rec["game_plies"])
        assert torch.equal(got.actions.cpu(), rec["actions"]), t
        assert torch.equal(got.log_probs.cpu(), rec["log_probs"]), t
        g = mo == 0                                          # the greedy model: the arg-max over the recorded mask
        if bool(g.any()):
            best = logits.masked_fill(~_masks(bits), float("-inf")).argmax(dim=1)
            assert torch.equal(best[g].cpu(), rec["actions"][g.cpu()]), t
            assert float(rec["log_probs"][g.cpu()].abs().max()) <= 2e-7
        greedy_rows += int(g.sum())
        neutral_rows += int((mo == 1).sum())
        late += int((rec["game_plies"] > 0).sum())
    assert greedy_rows > 50 and neutral_rows > 50 and late > 50
    # the game ply is 0 at the start of every game, restarted games included
    assert bool((recs[0]["game_plies"] == 0).all()) and int(max(r["game_plies"].max() for r in recs)) < MAX_PLY
    ended = (recs[-2]["terminated"] | recs[-2]["truncated"]).bool()
    if bool(ended.any()):
        assert bool((recs[-1]["game_plies"][ended] == 0).all())


# ------------------------------------------------------------------ greedy play under the graph
def test_greedy_games_of_a_pairing_are_identical_under_the_graph():
    arena = MatchArena(_group(), N, PER, MAX_PLY, sync_every=4, graph=True, seed=5, game_log=512, sampling=GREEDY)
    results, stats = arena.run_round(PAIRINGS, games_per_match=16)
    assert stats.games_dropped == 0
    assert _all_identical(results)


def test_set_sampling_applies_without_a_new_capture():
    arena = MatchArena(_group(), N, PER, MAX_PLY, sync_every=4, graph=True, seed=6, game_log=512, sampling=NEUTRAL)
    results, _ = arena.run_round(PAIRINGS, games_per_match=16)
    assert not _all_identical(results)                       # temperature 1: the games of a pairing differ
    graph, table = arena._graph, arena._ctl
    assert graph is not None
    arena.set_sampling(GREEDY)
    results, _ = arena.run_round(PAIRINGS, games_per_match=16)
    assert _all_identical(results)
    assert arena._graph is graph and arena._ctl is table
    arena.set_sampling(None)                                 # neutral rows, still the same table
    assert arena._ctl is table and np.array_equal(table.cpu().numpy(), controls_table(None, 2))
    arena.set_sampling([SamplingControls(0.5), GREEDY])
    assert np.array_equal(table.cpu().numpy(), controls_table([SamplingControls(0.5), GREEDY], 2))
    with pytest.raises(ValueError, match="expected 2"):
        arena.set_sampling([GREEDY])


def test_opening_plies_are_sampled_and_the_rest_is_greedy():
    ctl = SamplingControls(temperature=0, opening_temperature=1, opening_plies=6)
    arena = MatchArena(_group(), N, PER, MAX_PLY, sync_every=4, graph=True, seed=7, game_log=512, sampling=ctl)
    results, stats = arena.run_round(PAIRINGS, games_per_match=16)
    assert stats.games_dropped == 0
    prefixes = set()
    for games in _own_games(results):
        assert len(games) >= 2
        by_prefix = {}
        for g in games:
            assert len(g) > 6
            by_prefix.setdefault(g[:6], set()).add(g)
        assert all(len(v) == 1 for v in by_prefix.values())  # the same six first moves: the same game
        prefixes |= set(by_prefix)
    assert len(prefixes) >= 2


def test_graph_equals_no_graph_under_controls():
    ctl = [SamplingControls(0.5, top_k=5), SamplingControls(0.0, 1.0, 6)]
    eager = MatchArena(_group(), N, PER, MAX_PLY, sync_every=2, graph=False, seed=11, sampling=ctl)
    graph = MatchArena(_group(), N, PER, MAX_PLY, sync_every=2, graph=True, seed=11, sampling=ctl)
    r1, s1 = eager.run_round(PAIRINGS, games_per_match=8)
    r2, s2 = graph.run_round(PAIRINGS, games_per_match=8)
    assert _key(r1) == _key(r2) and s1.round_plies == s2.round_plies
    assert torch.equal(eager.env.current().observations, graph.env.current().observations)


def test_refusals():
    with pytest.raises(ValueError, match="collect=True"):
        MatchArena(_group(), N, PER, MAX_PLY, collect=True, sampling=GREEDY)
    with pytest.raises(ValueError, match="expected 2"):
        MatchArena(_group(), N, PER, MAX_PLY, sampling=[GREEDY, NEUTRAL, NEUTRAL])
    plain = MatchArena(_group(), N, PER, MAX_PLY, graph=False)
    assert plain._ctl is None
    with pytest.raises(ValueError, match="built without sampling"):
        plain.set_sampling(GREEDY)


# ------------------------------------------------------------------ the league rollout
def _roll(opponent_sampling, K=3):
    ms = _models(K + 1)
    return LeagueRollout(ms[0], ms[1:], [10 * k + 3 for k in range(K)], num_envs=N, max_ply=MAX_PLY,
                         value_adapter=MultiHeadValueAdapter(score_blend_alpha=0.25), color_randomization=True,
                         opponent_weights=[1.0, 2.0, 1.0][:K], seed=4242, graph=False, record=True, sync_every=4,
                         opponent_sampling=opponent_sampling)


def _replay(roll, rec):
    """the recorded ply through ka_policy_sample, the plain sampler: (logits, actions, log-probs)"""
    obs, bits = rec["obs"].to(DEV), rec["mask_bits"].to(DEV)
    mo = torch.from_numpy(rec["model_of"]).to(DEV)
    out = roll.group.forward(obs, mo)
    logits = out.policy_logits.reshape(N, -1).contiguous()
    act, lp, val = torch.empty(N, dtype=torch.int64, device=DEV), torch.empty(N, device=DEV), torch.empty(N, device=DEV)
    nl, fl = torch.empty(N, dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    _lib.call("ka_policy_sample", logits, 0, bits, MASK_WORDS, rec["seed"], out.value_logits,
              out.score_lead.reshape(N).contiguous(), roll.alpha, act, lp, val, nl, fl, N, ACTION_SPACE, _stream())
    return logits, bits, mo, act.cpu().numpy(), lp.cpu().numpy()


def _term_values(roll, rec):
    out = np.full(N, np.nan, np.float32)
    envs = rec["terminal_envs"]
    if len(envs):
        o = roll.group.forward(rec["terminal_obs"].to(DEV), torch.zeros(len(envs), dtype=torch.int32, device=DEV))
        v = torch.empty(len(envs), device=DEV)
        _lib.call("ka_scalar_value", o.value_logits.contiguous(), o.score_lead.reshape(-1).contiguous(), roll.alpha, v,
                  len(envs), _stream())
        out[envs] = v.cpu().numpy()
    return out


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def test_league_opponents_play_greedy_and_the_learner_keeps_its_own_draws():
    roll = _roll(GREEDY)
    assert roll._ctl is not None and np.array_equal(roll._ctl.cpu().numpy()[0], NEUTRAL.row())
    buf = KataGoRolloutBuffer(N, OBS, ACTION_SPACE, device=DEV)
    roll.collect(buf, 12)
    learner_rows = opponent_rows = 0
    for t, rec in enumerate(roll.record):
        logits, bits, mo, act, lp = _replay(roll, rec)
        mine = rec["model_of"] == 0
        assert np.array_equal(act[mine], rec["actions"][mine]), t         # the learner: the plain sampler, bit for bit
        assert _bits_equal(lp[mine], rec["log_probs"][mine]), t
        best = logits.masked_fill(~_masks(bits), float("-inf")).argmax(dim=1).cpu().numpy()
        assert np.array_equal(best[~mine], rec["actions"][~mine]), t      # every opponent: the arg-max of its own logits
        learner_rows += int(mine.sum())
        opponent_rows += int((~mine).sum())
    assert learner_rows > 40 and opponent_rows > 40
    # the buffer holds the learner's recorded actions and log-probs: the host restatement of the epoch over the records
    recs = [dict(r, term_values=_term_values(roll, r)) for r in roll.record]
    want, _ = _league_host(recs, num_envs=N, obs_shape=OBS, action_space=ACTION_SPACE, opponent_ids=roll.opponent_ids,
                           seed=roll._draw_seed, cum=roll._cum_host, color_randomization=True, score_norm=roll.score_norm,
                           side=roll.record[0]["side"], opp=roll.record[0]["opp"], games=np.zeros(N, np.int64))
    got = buf.flatten()
    assert buf.size == want["size"] and got["actions"].numel() > 40
    assert np.array_equal(got["actions"].cpu().numpy(), np.asarray(want["actions"]))
    assert _bits_equal(got["log_probs"].cpu().numpy(), want["log_probs"])
    # every log-prob in the buffer is one the plain sampler gave a learner row
    seen = {float(x) for rec in roll.record for x in rec["log_probs"][rec["model_of"] == 0]}
    assert {float(x) for x in got["log_probs"].cpu().numpy()} <= seen


def test_league_without_the_option_keeps_the_play_sampler():
    roll = _roll(None)
    assert roll._ctl is None
    buf = KataGoRolloutBuffer(N, OBS, ACTION_SPACE, device=DEV)
    roll.collect(buf, 8)
    for t, rec in enumerate(roll.record):
        _, _, _, act, lp = _replay(roll, rec)
        assert np.array_equal(act, rec["actions"]) and _bits_equal(lp, rec["log_probs"]), t


def test_set_opponents_keeps_a_single_control_and_resets_a_list_of_another_size():
    roll = _roll(GREEDY, K=2)
    ms = _models(4)
    roll.set_opponents(ms[1:4], [3, 13, 23])                               # one control for all: kept
    assert np.array_equal(roll._ctl.cpu().numpy(), np.concatenate([controls_table(None, 1), controls_table(GREEDY, 3)]))
    per = [GREEDY, SamplingControls(2.0), SamplingControls(0.5, top_k=4)]
    roll.set_opponents(ms[1:4], [3, 13, 23], sampling=per)
    assert np.array_equal(roll._ctl.cpu().numpy()[1:], controls_table(per, 3))
    roll.set_opponents(ms[1:4], [3, 13, 23])                               # same size: the list stays
    assert np.array_equal(roll._ctl.cpu().numpy()[1:], controls_table(per, 3))
    roll.set_opponents(ms[1:3], [3, 13])                                   # another size: neutral
    assert roll._ctl is None
    with pytest.raises(ValueError, match="one per opponent"):
        roll.set_opponents(ms[1:3], [3, 13], sampling=per)
