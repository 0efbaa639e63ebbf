"""Rollout collection inside the arena's ply: ka_arena_record_pre / ka_arena_record_post against a numpy restatement on
synthetic ply data (bit for bit, with a guard band behind the store), and whole rounds of MatchArena(collect=True) against
the rows selected from the host records, with and without a captured graph."""
import numpy as np
import pytest
import torch

from keisei_amd import _lib
from keisei_amd.shogi_gym import MASK_WORDS
from keisei_amd.training import MatchArena
from keisei_amd.training.match_arena import _rollout_rows_host
from keisei_amd.training.model_group import SEResNetGroup
from keisei_amd.training.models.se_resnet import SEResNetModel, SEResNetParams
from oracle import keisei_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPE = orc.NetShape(2, 128, 8, 64, 16, 128, 64)
MAX_PLY = 40
OBS = 50 * 81
PAIRINGS = [(0, 1), (2, 0), (1, 1), (3, 2), (0, 3)]
BITS = {0: 1, 1: 2, 2: 3, 4: 1}                              # pairing 3 is not trainable; 2 collects both sides
GUARD, PATTERN = 3, 0x7FC0A5A5
_GROUP = {}


def _group(K=4):
    if K not in _GROUP:
        ms = []
        for k in range(K):
            m = SEResNetModel(SEResNetParams(**SHAPE.__dict__))
            m.load_state_dict(orc.init_like_state_dict(SHAPE, salt=29 * k + 5), strict=True)
            ms.append(m.to(DEV).eval())
        _GROUP[K] = SEResNetGroup(ms)
    return _GROUP[K]


# ------------------------------------------------------------------ 5. the kernels
def _run_kernels(S, E, cap, plies, status, bits):
    """plies: list of dicts of numpy arrays over the S*E envs.  Returns the store, the cursors and the guard check."""
    N = S * E
    state = torch.zeros(8 + 8 * S, dtype=torch.int32)
    state[8:].view(S, 8)[:, 7] = torch.tensor(status, dtype=torch.int32)
    state = state.to(DEV)
    side_bits = torch.tensor(bits, dtype=torch.int32, device=DEV)
    cursors = torch.zeros(4 * S, dtype=torch.int32, device=DEV)
    row_of = torch.full((N,), -7, dtype=torch.int32, device=DEV)
    R = S * cap
    fo = torch.full((R + GUARD, OBS), PATTERN, dtype=torch.int32, device=DEV)
    fm = torch.full((R + GUARD, MASK_WORDS), PATTERN, dtype=torch.int32, device=DEV)
    fa = torch.full((R + GUARD,), PATTERN, dtype=torch.int64, device=DEV)
    fp = torch.full((R + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    fr = torch.full((R + GUARD,), PATTERN, dtype=torch.int32, device=DEV)
    fd = torch.full((R + GUARD,), PATTERN, dtype=torch.int32, device=DEV)
    st = _lib.stream_ptr()
    for p in plies:
        t = {k: torch.from_numpy(v).to(DEV) for k, v in p.items()}
        _lib.call("ka_arena_record_pre", state, side_bits, S, E, t["obs"], t["mask"], t["actions"], t["pre"], t["nlegal"],
                  cursors, row_of, fo.view(torch.float32), fm, fa, fp, cap, OBS, MASK_WORDS, st)
        _lib.call("ka_arena_record_post", cursors, row_of, S, E, t["rewards"], t["term"], t["trunc"], fr.view(torch.float32),
                  fd.view(torch.float32), cap, st)
    torch.cuda.synchronize()
    intact = all(bool((f[R:] == v).all()) for f, v in ((fo, PATTERN), (fm, PATTERN), (fa, PATTERN), (fp, 0xA5), (fr, PATTERN),
                                                        (fd, PATTERN)))
    store = {"obs": fo[:R].cpu().numpy(), "mask": fm[:R].cpu().numpy(), "actions": fa[:R].cpu().numpy(),
             "persp": fp[:R].cpu().numpy(), "rewards": fr[:R].cpu().numpy(), "dones": fd[:R].cpu().numpy()}
    return store, cursors.cpu().numpy().reshape(S, 4), intact


def _host_rows(S, E, cap, plies, status, bits):
    """numpy restatement: per slot the list of (ply, env) rows offered, in (ply, env) order"""
    rows = [[] for _ in range(S)]
    for t, p in enumerate(plies):
        for s in range(S):
            if not (status[s] & 1) or (status[s] & 2) or not (bits[s] & 3):
                continue
            envs = range(s * E, (s + 1) * E)
            if any(p["nlegal"][e] == 0 for e in envs):
                continue
            rows[s] += [(t, e) for e in envs if (bits[s] >> int(p["pre"][e])) & 1]
    return rows


def _synthetic(S, E, T, seed):
    rng = np.random.default_rng(seed)
    N = S * E
    plies = []
    for t in range(T):
        plies.append({"obs": rng.standard_normal((N, 50, 9, 9)).astype(np.float32),
                      "mask": rng.integers(-2 ** 31, 2 ** 31, (N, MASK_WORDS)).astype(np.int32),
                      "actions": rng.integers(0, 11259, N).astype(np.int64),
                      "pre": rng.integers(0, 2, N).astype(np.uint8), "nlegal": np.full(N, 9, np.int32),
                      "rewards": rng.choice([-1.0, 0.0, 1.0], N).astype(np.float32),
                      "term": rng.random(N) < 0.3, "trunc": rng.random(N) < 0.2})
    return plies


def _check_store(store, cur, rows, plies, cap):
    f32 = lambda a: a.view(np.float32)  # noqa: E731
    for s, offered in enumerate(rows):
        fit = offered[:cap]
        assert cur[s, 0] == len(fit) and cur[s, 1] == 0 and cur[s, 2] == len(offered) - len(fit), (s, cur[s])
        for r, (t, e) in enumerate(fit):
            p, row = plies[t], s * cap + r
            assert np.array_equal(store["obs"][row], p["obs"][e].reshape(-1).view(np.int32)), (s, r)
            assert np.array_equal(store["mask"][row], p["mask"][e])
            assert store["actions"][row] == p["actions"][e] and store["persp"][row] == p["pre"][e]
            assert f32(store["rewards"])[row] == p["rewards"][e]
            assert f32(store["dones"])[row] == float(p["term"][e] or p["trunc"][e])
        for row in range(s * cap + len(fit), (s + 1) * cap):                    # the rest of the region is untouched
            assert store["actions"][row] == PATTERN and store["rewards"][row] == PATTERN


def test_record_kernels_match_the_restatement():
    S, E, T = 6, 5, 4
    status = [1, 1, 1, 0, 3, 1]                              # slot 3 unseated, slot 4 done
    bits = [1, 2, 3, 3, 3, 3]
    plies = _synthetic(S, E, T, 1)
    plies[1]["nlegal"][5 * E + 2] = 0                        # slot 5 records nothing at ply 1
    cap = T * E
    store, cur, intact = _run_kernels(S, E, cap, plies, status, bits)
    rows = _host_rows(S, E, cap, plies, status, bits)
    assert intact
    assert [len(r) for r in rows][2] == T * E and len(rows[3]) == 0 and len(rows[4]) == 0 and len(rows[5]) == 3 * E
    assert 0 < len(rows[0]) < T * E and len(rows[0]) + len(rows[1]) > 0
    _check_store(store, cur, rows, plies, cap)


def test_record_kernels_large_slot_and_small_capacity():
    S, E, T = 2, 300, 3                                      # a slot wider than one workgroup's scan tile
    status, bits = [1, 1], [1, 3]                       # the last slot overflows: towards the guard band
    plies = _synthetic(S, E, T, 2)
    cap = 2 * E + 17                                         # the third ply does not fit
    store, cur, intact = _run_kernels(S, E, cap, plies, status, bits)
    rows = _host_rows(S, E, cap, plies, status, bits)
    assert intact, "a row beyond the capacity was written"
    assert len(rows[1]) == 3 * E and cur[1, 2] == 3 * E - cap and cur[0, 2] == 0
    _check_store(store, cur, rows, plies, cap)


# ------------------------------------------------------------------ 6.-7. in the arena
def _key(results):
    return [(r.a, r.b, r.a_wins, r.b_wins, r.draws, r.plies, r.partial) for r in results]


def _round(graph, sync_every, record=False, collect=True, trainable=BITS):
    arena = MatchArena(_group(), 12, 4, MAX_PLY, sync_every=sync_every, graph=graph, seed=11, record=record, collect=collect)
    results, stats = arena.run_round(PAIRINGS, games_per_match=6, **({"trainable": trainable} if collect else {}))
    return arena, results, stats


def _same_rollout(a, b):
    for k in ("observations", "actions", "rewards", "dones", "perspective", "legal_mask_bits"):
        if not torch.equal(getattr(a, k), getattr(b, k)):
            return False
    return True


@pytest.fixture(scope="module")
def recorded():
    return _round(False, 2, record=True)


def test_rollouts_are_the_rows_of_the_host_records(recorded):
    arena, results, stats = recorded
    recs = [{k: (v.numpy() if isinstance(v, torch.Tensor) else v) for k, v in r.items()} for r in arena.record]
    bits = [BITS.get(i, 0) for i in range(len(PAIRINGS))]
    rows = _rollout_rows_host(recs, PAIRINGS, bits, num_slots=3, envs_per_slot=4, games_per_match=6, max_ply=MAX_PLY,
                              sync_every=2)
    total = 0
    for i, (res, want) in enumerate(zip(results, rows)):
        if not bits[i]:
            assert res.rollout is None and not want
            continue
        ro = res.rollout
        assert ro is not None and ro.legal_masks is None and len(want) == ro.actions.shape[0] > 0, i
        for k in ("observations", "actions", "rewards", "dones", "perspective", "legal_mask_bits"):
            assert getattr(ro, k).device.type == "cuda", k
        pick = lambda key: torch.from_numpy(np.stack([recs[a][key][b] for a, b in want]))  # noqa: E731
        assert torch.equal(ro.observations.cpu(), pick("obs")), i
        assert torch.equal(ro.legal_mask_bits.cpu(), pick("mask_bits")), i
        assert torch.equal(ro.actions.cpu(), pick("actions")) and torch.equal(ro.perspective.cpu(), pick("pre_players"))
        assert torch.equal(ro.rewards.cpu(), pick("rewards"))
        assert torch.equal(ro.dones.cpu(), (pick("terminated") | pick("truncated")).float())
        sides = set(ro.perspective.cpu().tolist())
        assert sides == ({0} if bits[i] == 1 else {1} if bits[i] == 2 else {0, 1}), i
        if bits[i] & 2:                                     # games end by truncation at the even MAX_PLY: player 1 moved last
            assert float(ro.dones.sum()) > 0
        total += len(want)
    assert stats.rollout_rows == total and stats.rollouts_dropped == 0


def test_collection_does_not_change_the_results(recorded):
    _, results, stats = recorded
    _, plain, plain_stats = _round(False, 2, collect=False)
    assert _key(plain) == _key(results) and plain_stats.round_plies == stats.round_plies
    assert all(r.rollout is None for r in plain)


@pytest.mark.parametrize("sync_every", [2, 4])
def test_graph_gives_the_same_rollouts(recorded, sync_every):
    eager = recorded[1] if sync_every == 2 else _round(False, sync_every)[1]
    arena, graphed, _ = _round(True, sync_every)
    assert _key(graphed) == _key(eager)
    for a, b in zip(eager, graphed):
        assert (a.rollout is None) == (b.rollout is None)
        assert a.rollout is None or _same_rollout(a.rollout, b.rollout)
    again, _ = arena.run_round(PAIRINGS, games_per_match=6, trainable=BITS)      # a second round on the same graph
    assert _key(again) == _key(graphed)
    assert all(a.rollout is None or _same_rollout(a.rollout, b.rollout) for a, b in zip(graphed, again))
    none, _ = arena.run_round(PAIRINGS, games_per_match=6)                        # collection built in, nothing trainable
    assert _key(none) == _key(graphed) and all(r.rollout is None for r in none)


def test_trainable_needs_collect():
    arena = MatchArena(_group(), 8, 4, MAX_PLY, sync_every=2, graph=False)
    with pytest.raises(ValueError, match="collect=True"):
        arena.run_round([(0, 1)], games_per_match=2, trainable={0: 1})
