"""Per-game style features inside the arena's ply: ka_arena_features_step / ka_arena_features_seat against the host
GameFeatureTracker on synthetic plies (records, cursors and accumulators word for word, with a guard band behind the
store), and whole rounds of MatchArena(features=True) against _features_host on the arena's own records, with and
without a captured graph, with and without rollout collection."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch

from keisei_amd import _lib
from keisei_amd.training import GameFeatureAccumulator, GameFeatureTracker, MatchArena
from keisei_amd.training.game_feature_tracker import ACC_WORDS, RECORD_WORDS
from keisei_amd.training.match_arena import _features_host
from keisei_amd.training.model_group import SEResNetGroup
from keisei_amd.training.models.se_resnet import SEResNetModel, SEResNetParams
from oracle import keisei_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPE = orc.NetShape(2, 128, 8, 64, 16, 128, 64)
MAX_PLY = 40
PAIRINGS = [(0, 1), (2, 0), (1, 1), (3, 2), (0, 3)]
GUARD, PATTERN = 3, 0x7FC0A5A5
STEP_KEYS = ("actions", "captured_piece", "termination_reason", "ply_count", "pre_players", "terminated", "truncated", "rewards")
_GROUP = {}


def _tool():
    path = Path(__file__).resolve().parent.parent / "tools" / "make_features_golden.py"
    spec = importlib.util.spec_from_file_location("make_features_golden", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


TOOL = _tool()


def _group(K=4):
    if K not in _GROUP:
        ms = []
        for k in range(K):
            m = SEResNetModel(SEResNetParams(**SHAPE.__dict__))
            m.load_state_dict(orc.init_like_state_dict(SHAPE, salt=29 * k + 5), strict=True)
            ms.append(m.to(DEV).eval())
        _GROUP[K] = SEResNetGroup(ms)
    return _GROUP[K]


# ------------------------------------------------------------------ 6. the kernels
def _run_kernels(S, E, cap, plies, status, first_ply=100):
    """plies: per ply a dict of numpy arrays over the S*E envs (STEP_KEYS and nlegal).  Returns the record store, the
    cursors, the accumulators and the guard check."""
    N = S * E
    state = torch.zeros(8 + 8 * S, dtype=torch.int32)
    state[8:].view(S, 8)[:, 7] = torch.tensor(status, dtype=torch.int32)
    state = state.to(DEV)
    acc = torch.full((N * ACC_WORDS + GUARD,), PATTERN, dtype=torch.int32, device=DEV)
    records = torch.full((S * cap + GUARD, RECORD_WORDS), PATTERN, dtype=torch.int32, device=DEV)
    cursors = torch.zeros(2 * S, dtype=torch.int32, device=DEV)
    jobs = torch.zeros(S + 2, 4, dtype=torch.int32)
    jobs[:S, 0] = torch.arange(S, dtype=torch.int32)
    jobs[S, 0], jobs[S + 1, 0] = S, -1                       # rows naming no slot are skipped
    jobs = jobs.to(DEV)
    st = _lib.stream_ptr()
    _lib.call("ka_arena_features_seat", jobs, S + 2, S, E, acc, st)
    for t, p in enumerate(plies):
        state[2:3].fill_(first_ply + t)
        d = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in p.items() if k != "ply_count"}
        ply = torch.from_numpy(p["ply_count"].astype(np.uint16).view(np.int16)).to(DEV)     # as VecEnv hands it over
        _lib.call("ka_arena_features_step", state, S, E, d["actions"], d["pre_players"], d["nlegal"], d["captured_piece"],
                  d["termination_reason"], ply, d["rewards"], d["terminated"], d["truncated"], acc, records, cursors, cap, st)
    torch.cuda.synchronize()
    intact = bool((acc[N * ACC_WORDS:] == PATTERN).all()) and bool((records[S * cap:] == PATTERN).all())
    return (records[:S * cap].cpu().numpy().reshape(S, cap, RECORD_WORDS), cursors.cpu().numpy().reshape(S, 2),
            acc[:N * ACC_WORDS].cpu().numpy().reshape(S, E, ACC_WORDS), intact)


def _mirror(S, E, plies, status, first_ply=100):
    """one host tracker per slot under the referee's rule: seated, not done, no env of the slot without a legal action.
    Returns per slot the expected records (env index and round ply as the device writes them) and accumulator words."""
    trackers = [GameFeatureTracker(E, 0, 1, 0) for _ in range(S)]
    expect = [[] for _ in range(S)]
    for t, p in enumerate(plies):
        for s in range(S):
            lo, hi = s * E, (s + 1) * E
            if not (status[s] & 1) or (status[s] & 2) or (p["nlegal"][lo:hi] == 0).any():
                continue
            before = len(trackers[s].records)
            trackers[s].record_step(*(p[k][lo:hi] for k in STEP_KEYS))
            for rec in trackers[s].records[before:]:
                rec = rec.copy()
                rec[0] += lo
                rec[7] = first_ply + t
                expect[s].append(rec)
    words = np.array([[a.words() for a in tr.accumulators] for tr in trackers], np.int32)
    return expect, words


def _synthetic(S, E, T, seed, p_done=0.05):
    plies = TOOL.synthetic_stream(S * E, T, seed, p_done=p_done)
    for p in plies:
        p["nlegal"] = np.full(S * E, 9, np.int32)
    return plies


def _check(S, cap, got, expect, words):
    records, cur, acc, intact = got
    assert intact, "a word behind the store or behind the accumulators was written"
    assert np.array_equal(acc, words)
    for s in range(S):
        fit = expect[s][:cap]
        assert (cur[s, 0], cur[s, 1]) == (len(fit), len(expect[s]) - len(fit)), (s, cur[s], len(expect[s]))
        if fit:
            assert np.array_equal(records[s, :len(fit)], np.array(fit, np.int32)), s
        assert (records[s, len(fit):] == PATTERN).all(), s   # the rest of the region is untouched


def test_features_kernel_matches_the_host_tracker():
    S, E, T = 6, 5, 60
    status = [1, 1, 1, 0, 3, 1]                              # slot 3 unseated, slot 4 done
    plies = _synthetic(S, E, T, 1)
    plies[7]["nlegal"][5 * E + 2] = 0                        # slot 5 records nothing at ply 7
    plies[7]["terminated"][5 * E:6 * E] = True               # ... not even the games that end there
    cap = T * E
    got = _run_kernels(S, E, cap, plies, status)
    expect, words = _mirror(S, E, plies, status)
    assert [len(e) > 3 for e in expect] == [True, True, True, False, False, True] and not expect[3] and not expect[4]
    assert all(rec[7] != 107 for rec in expect[5])
    assert max(rec[1] for rec in expect[0]) > 32767          # env 0's ply count is read unsigned
    assert {rec[4] for e in expect for rec in e} == {-1, 0, 1} and {rec[2] for e in expect for rec in e} == set(range(6))
    fresh = np.array(GameFeatureAccumulator().words(), np.int32)
    assert (words[3] == fresh).all() and (words[4] == fresh).all() and (words[0] != fresh).any()
    _check(S, cap, got, expect, words)


def test_features_kernel_wide_slot_and_small_capacity():
    S, E, T = 2, 300, 6                                      # a slot wider than the workgroup's 256 threads
    plies = _synthetic(S, E, T, 2, p_done=0.3)
    cap = 200                                                # fewer records than games finish: towards the guard band
    got = _run_kernels(S, E, cap, plies, [1, 1])
    expect, words = _mirror(S, E, plies, [1, 1])
    assert all(len(e) > cap + 100 for e in expect)
    assert any(rec[0] % E >= 256 for rec in expect[1][:cap])  # records of envs of the second tile inside the kept ones
    _check(S, cap, got, expect, words)
    assert got[1][1, 1] == len(expect[1]) - cap > 0


# ------------------------------------------------------------------ 7.-8. in the arena
def _key(results):
    return [(r.a, r.b, r.a_wins, r.b_wins, r.draws, r.plies, r.partial) for r in results]


def _rows(results):
    return [[row.to_dict() for row in r.feature_tracker.completed_rows] for r in results]


def _round(graph, sync_every, record=False, collect=False, features=True, **kw):
    arena = MatchArena(_group(), 12, 4, MAX_PLY, sync_every=sync_every, graph=graph, seed=11, record=record, collect=collect,
                       features=features)
    if collect:
        kw["trainable"] = {0: 1, 1: 2, 2: 3, 4: 1}
    results, stats = arena.run_round(PAIRINGS, games_per_match=6, **kw)
    return arena, results, stats


@pytest.mark.parametrize("sync_every", [1, 4])
def test_round_features_are_the_host_trackers_rows_on_the_arenas_records(sync_every):
    ids = {0: 40, 1: 41, 2: 42, 3: 43}
    arena, results, stats = _round(False, sync_every, record=True, entry_ids=ids, epoch=7)
    recs = [{k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()} for r in arena.record]
    want = _features_host(recs, PAIRINGS, num_slots=3, envs_per_slot=4, games_per_match=6, max_ply=MAX_PLY,
                          sync_every=sync_every, entry_ids=ids, epoch=7)
    total = 0
    for i, (res, tr) in enumerate(zip(results, want)):
        got = res.feature_tracker
        assert isinstance(got, GameFeatureTracker) and (got.entry_a_id, got.entry_b_id, got.epoch) == (ids[res.a], ids[res.b], 7)
        assert len(got.completed_rows) == 2 * res.games > 0, i
        assert [r.to_dict() for r in got.completed_rows] == [r.to_dict() for r in tr.completed_rows], i
        assert got.records.shape == (res.games, RECORD_WORDS) and got.records.dtype == np.int32
        slot = got.records[0, 0] // 4
        assert np.array_equal(got.records[:, 0] - 4 * slot, tr.records[:, 0]) and (np.diff(got.records[:, 7]) >= 0).all()
        assert np.array_equal(got.records[:, 1:7], tr.records[:, 1:7]) and np.array_equal(got.records[:, 8:], tr.records[:, 8:])
        total += len(got.completed_rows)
    assert stats.feature_rows == total and stats.features_dropped == 0
    assert all(r["ply_count"].max() == MAX_PLY and r["captured_piece"].dtype == np.uint8 for r in recs[MAX_PLY - 1:MAX_PLY])


def test_graph_gives_the_same_features():
    _, eager, _ = _round(False, 4)
    arena, graphed, stats = _round(True, 4)
    assert _key(graphed) == _key(eager) and _rows(graphed) == _rows(eager)
    assert stats.feature_rows == sum(2 * r.games for r in graphed) > 0
    again, _ = arena.run_round(PAIRINGS, games_per_match=6)                       # a second round on the same graph
    assert _key(again) == _key(graphed) and _rows(again) == _rows(graphed)


def test_features_change_nothing_they_do_not_own():
    _, with_f, stats_f = _round(False, 2)
    _, plain, stats_p = _round(False, 2, features=False)
    assert _key(plain) == _key(with_f) and stats_p.round_plies == stats_f.round_plies
    assert all(r.feature_tracker is None for r in plain) and stats_p.feature_rows == 0
    _, both, _ = _round(False, 2, collect=True)
    _, coll, _ = _round(False, 2, collect=True, features=False)
    assert _key(both) == _key(coll) == _key(plain) and _rows(both) == _rows(with_f)
    for a, b in zip(both, coll):
        assert (a.rollout is None) == (b.rollout is None)
        if a.rollout is not None:
            for k in ("observations", "actions", "rewards", "dones", "perspective", "legal_mask_bits"):
                assert torch.equal(getattr(a.rollout, k), getattr(b.rollout, k)), k
    assert any(r.rollout is not None for r in both)


def test_entry_ids_must_cover_the_models_played():
    arena = MatchArena(_group(), 8, 4, MAX_PLY, sync_every=2, graph=False, features=True)
    with pytest.raises(ValueError, match="entry_ids"):
        arena.run_round([(0, 3)], games_per_match=2, entry_ids={0: 5})
    with pytest.raises(ValueError, match="entry_ids"):
        arena.run_round([(0, 3)], games_per_match=2, entry_ids=[5, 6, 7])
