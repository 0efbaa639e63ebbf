"""The game log inside the loops that play on the device: SelfPlayRollout(game_log=) and MatchArena(game_log=) against
games rebuilt on the host from the loops' own per-ply records, every game replayed move by move on the CPU oracle, the
schedule (graph, sync_every) leaving the games unchanged, the log leaving the rollout rows unchanged, and the way back:
recorded games -> DeviceSLDataset, directly and through a .sfen file."""
import gc

import numpy as np
import pytest
import torch

from keisei_amd.shogi_gym import ACTION_SPACE
from keisei_amd.sl.parsers import START_SFEN
from keisei_amd.sl.prepare import _value_of, dataset_from_recorded_games, prepare_sl_dataset
from keisei_amd.training import MatchArena, SelfPlayRollout, write_sfen_games
from keisei_amd.training.katago_ppo import KataGoRolloutBuffer
from keisei_amd.training.match_arena import _referee_host
from keisei_amd.training.model_group import SEResNetGroup
from keisei_amd.training.models.se_resnet import SEResNetModel, SEResNetParams
from oracle import keisei_oracle as orc
from oracle import shogi as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPE = orc.NetShape(2, 128, 8, 64, 16, 128, 64)
OBS = (50, 9, 9)
WHITE_SFEN = "lnsgkgsnl/1r5b1/ppppppppp/9/9/2P6/PP1PPPPPP/1B5R1/LNSGKGSNL w - 1"
N, MAX_PLY, STEPS = 5, 8, 24
_MODELS = {}


@pytest.fixture(autouse=True)
def _release_device_objects():
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


def _epoch(game_log, *, graph=False, record=False, sync_every=4, pool=None):
    roll = SelfPlayRollout(_model(), num_envs=N, max_ply=MAX_PLY, graph=graph, record=record, sync_every=sync_every, seed=1,
                           game_log=game_log, start_pool_capacity=4 if pool else 0)
    if pool:
        roll.env.set_start_sfens(pool, seed=3)
        roll.reset()
    buf = KataGoRolloutBuffer(N, OBS, ACTION_SPACE, device=DEV)
    stats = roll.collect(buf, STEPS)
    return roll, stats, {k: v.clone() for k, v in buf.flatten().items()}


_BASE = {}


def _base():
    """The recorded epoch every self-play test compares against: computed once."""
    if not _BASE:
        roll, stats, cols = _epoch(64, record=True)
        _BASE.update(records=roll.record, stats=stats, cols=cols)
    return _BASE


def _same_bits(a, b):
    if a.dtype.is_floating_point:                                # NaN cells compare by their bits
        return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


def _key(g):
    return (g.env, g.actions.tolist(), g.winner, g.reason, g.truncated, g.carried, g.black, g.white, g.end_ply, g.game_number,
            g.start_board.tobytes(), g.start_hands.tobytes(), g.start_side)


def _winner(reward, mover):
    return mover if reward > 0 else (1 - mover if reward < 0 else 2)


def _rebuild(records, pairing_of=None, pairings=None):
    """The games of per-ply records, in (ply, env) order, as (pairing, env, actions, winner, truncated-only, carried, ply,
    game number).  ``pairing_of[t][e]``: the pairing that plays env e at ply t, None for an env that is not live."""
    E = len(records[0]["actions"])
    moves, who, number, out = [[] for _ in range(E)], [[] for _ in range(E)], [0] * E, []
    for t, rec in enumerate(records):
        for e in range(E):
            p = 0 if pairing_of is None else pairing_of[t][e]
            moves[e].append(int(rec["actions"][e]))
            who[e].append(p)
            tm, tr = bool(rec["terminated"][e]), bool(rec["truncated"][e])
            if tm or tr:
                if p is not None:
                    out.append((p, e, moves[e], _winner(float(rec["rewards"][e]), int(rec["pre_players"][e])), tr and not tm,
                                any(q != p for q in who[e]), t, number[e]))
                moves[e], who[e], number[e] = [], [], number[e] + 1
    return out


def _replays_on_the_oracle(g, max_ply):
    """Every move legal, the game over at its last ply and not before, with the recorded reason and winner."""
    env = S.OracleVecEnv(1, max_ply)
    env.reset()
    env.set_state(0, g.start_board, g.start_hands, g.start_side)
    assert len(g.actions) >= 1
    for i, a in enumerate(g.actions):
        _, mask = env.observe(0)
        assert mask[int(a)], (g.env, g.game_number, i, int(a))
        r = env.step(np.asarray([int(a)]))
        done = bool(r["terminated"][0] or r["truncated"][0])
        assert done == (i == len(g.actions) - 1), (g.env, g.game_number, i)
    assert int(r["termination_reason"][0]) == g.reason
    assert bool(r["truncated"][0] and not r["terminated"][0]) == g.truncated
    assert _winner(float(r["rewards"][0]), (g.start_side + len(g.actions) - 1) & 1) == g.winner


# ---------------------------------------------------------------------------------------------- SelfPlayRollout
def test_selfplay_games_equal_the_rebuild_from_the_record_and_replay_on_the_oracle():
    base = _base()
    games, stats = base["stats"].games, base["stats"]
    want = _rebuild(base["records"])
    assert len(want) >= 15 and stats.games_dropped == 0
    assert [(0, g.env, g.actions.tolist(), g.winner, g.truncated, g.carried, g.end_ply, g.game_number) for g in games] == want
    assert len(games) == stats.terminated + stats.truncated
    assert all(g.is_standard_start and g.start_sfen() == START_SFEN and (g.black, g.white) == (-1, -1) for g in games)
    assert all(len(g.actions) <= MAX_PLY for g in games)
    for g in games:
        _replays_on_the_oracle(g, MAX_PLY)


@pytest.mark.parametrize("kw", [dict(graph=True, sync_every=4), dict(graph=False, sync_every=2)], ids=["graph-4", "eager-2"])
def test_one_seed_gives_the_same_games_whatever_the_schedule(kw):
    _, stats, cols = _epoch(64, **kw)
    assert [_key(g) for g in stats.games] == [_key(g) for g in _base()["stats"].games]
    assert stats.games_dropped == 0


def test_a_full_log_drops_whole_games_and_leaves_the_rows_alone():
    """The capacity holds between two sync points: of the games a chunk of sync_every plies finishes the first four (in
    (ply, env) order) are kept, the others counted."""
    base = _base()
    _, stats, cols = _epoch(4)
    by_chunk = {}
    for g in base["stats"].games:
        by_chunk.setdefault(g.end_ply // 4, []).append(g)
    kept = [g for c in sorted(by_chunk) for g in by_chunk[c][:4]]
    assert len(kept) < len(base["stats"].games)
    assert [_key(g) for g in stats.games] == [_key(g) for g in kept]
    assert stats.games_dropped == len(base["stats"].games) - len(kept)
    for k, v in base["cols"].items():
        assert _same_bits(v, cols[k]), k


def test_logging_changes_nothing_it_does_not_own():
    _, stats, cols = _epoch(0)
    assert stats.games == [] and stats.games_dropped == 0
    for k, v in _base()["cols"].items():
        assert _same_bits(v, cols[k]), k


def test_games_from_a_start_pool_carry_their_own_start():
    pool = [START_SFEN, WHITE_SFEN]
    roll, stats, _ = _epoch(64, pool=pool)
    roll.env.raise_if_refused()
    assert len(stats.games) >= 15
    starts = {g.start_sfen() for g in stats.games}
    assert starts == set(pool)
    assert {g.start_side for g in stats.games} == {0, 1}
    for g in stats.games:
        _replays_on_the_oracle(g, MAX_PLY)


# ---------------------------------------------------------------------------------------------- MatchArena
PAIRINGS = [(0, 1), (1, 0), (0, 1)]


@pytest.mark.parametrize("max_ply", [6, 5], ids=["max_ply6", "max_ply5"])
def test_match_arena_games(max_ply):
    """max_ply 6: the games of a slot end on a sync point, so the third pairing inherits fresh games.  max_ply 5: they end
    one ply before it, the slot idles for a ply and the third pairing inherits games in progress -- carried games.
    The referee tallies every game that ends in a live slot (overshoot included) and the log commits exactly those, so a
    result's recorded games are as many as its wins and draws, winner by winner."""
    group = SEResNetGroup([_model(5), _model(34)])
    arena = MatchArena(group, 8, 4, max_ply, sync_every=2, graph=False, record=True, seed=11, game_log=64)
    results, stats = arena.run_round(PAIRINGS, games_per_match=4)
    assert stats.games_dropped == 0 and len(results) == 3
    records = [{k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in rec.items()} for rec in arena.record]
    trace = []
    _referee_host(records, PAIRINGS, num_slots=2, envs_per_slot=4, games_per_match=4, max_ply=max_ply, sync_every=2, trace=trace)
    pairing_of = [[stepped.get(e // 4) for e in range(8)] for stepped in trace]
    for t, rec in enumerate(records):                            # the trace is the record's seating
        assert [p is not None for p in pairing_of[t]] == (rec["model_of"] >= 0).tolist()
    want = _rebuild(records, pairing_of)
    for p, r in enumerate(results):
        games = r.recorded_games
        assert len([g for g in games if not g.carried]) + len([g for g in games if g.carried]) == r.a_wins + r.b_wins + r.draws
        assert (r.a_wins, r.b_wins, r.draws) == tuple(sum(g.winner == w for g in games) for w in (0, 1, 2))
        assert all((g.black, g.white) == PAIRINGS[p] == (r.a, r.b) for g in games)
        assert [(p, g.env, g.actions.tolist(), g.winner, g.truncated, g.carried, g.end_ply, g.game_number) for g in games] == \
            [w for w in want if w[0] == p]
        assert r.games == len(games) > 0
        for g in games:
            assert g.is_standard_start
            _replays_on_the_oracle(g, max_ply)
    carried = [g for r in results for g in r.recorded_games if g.carried]
    assert bool(carried) == (max_ply == 5)
    plain = MatchArena(group, 8, 4, max_ply, sync_every=2, graph=False, seed=11)
    again, _ = plain.run_round(PAIRINGS, games_per_match=4)
    assert all(r.recorded_games is None for r in again)
    assert [(r.a_wins, r.b_wins, r.draws, r.plies) for r in again] == [(r.a_wins, r.b_wins, r.draws, r.plies) for r in results]


def test_match_arena_games_under_a_graph_and_from_a_pool():
    group = SEResNetGroup([_model(5), _model(34)])
    eager = MatchArena(group, 8, 4, 6, sync_every=2, graph=False, seed=11, game_log=64, start_pool_capacity=4)
    graphed = MatchArena(group, 8, 4, 6, sync_every=2, graph=True, seed=11, game_log=64, start_pool_capacity=4)
    out = []
    for arena in (eager, graphed):
        arena.env.set_start_sfens([START_SFEN, WHITE_SFEN], seed=3)
        results, stats = arena.run_round(PAIRINGS, games_per_match=4)
        assert stats.games_dropped == 0
        out.append([[_key(g) for g in r.recorded_games] for r in results])
        assert all(len(r.recorded_games) == r.games for r in results)
        assert {g.start_sfen() for r in results for g in r.recorded_games} == {START_SFEN, WHITE_SFEN}
    assert out[0] == out[1]


# ---------------------------------------------------------------------------------------------- back to SL data
def test_recorded_games_become_an_sl_dataset(tmp_path):
    base = _base()
    games, records = base["stats"].games, base["records"]
    ds, meta = dataset_from_recorded_games(games, batch_envs=16, max_moves=MAX_PLY)
    total = sum(len(g.actions) for g in games)
    assert len(ds) == total == meta["num_positions"] and meta["num_games"] == len(games)
    assert meta["games_nonstandard_start"] == meta["games_cut_illegal"] == meta["games_cut_by_rules"] == 0
    got = ds.read_batch(np.arange(total))
    policy = np.concatenate([g.actions.astype(np.int64) for g in games])
    value = np.asarray([_value_of(g.winner, i & 1) for g in games for i in range(len(g.actions))], np.int64)
    seen = torch.stack([records[g.end_ply - len(g.actions) + 1 + i]["obs"][g.env] for g in games for i in range(len(g.actions))])
    assert np.array_equal(got["policy_target"].cpu().numpy(), policy)
    assert np.array_equal(got["value_target"].cpu().numpy(), value)
    assert torch.equal(got["observation"].cpu().view(torch.int32), seen.view(torch.int32))
    # through the text: the same packed rows
    assert write_sfen_games(tmp_path / "games.sfen", games) == len(games)
    via_text, meta2 = prepare_sl_dataset([str(tmp_path)], min_ply=1, batch_envs=16, max_moves=MAX_PLY)
    assert meta2["num_positions"] == total and torch.equal(via_text.packed, ds.packed)
    # a game from another start is counted, not replayed
    other, meta3 = dataset_from_recorded_games([games[0], _from_white(games[1])], batch_envs=4, max_moves=MAX_PLY)
    assert meta3["games_nonstandard_start"] == 1 and len(other) == len(games[0].actions)


def _from_white(g):
    from dataclasses import replace

    return replace(g, start_side=1)
