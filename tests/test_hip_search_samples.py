"""The search samples on the GPU: ``ka_search_sample_step`` against its numpy restatement after every launch (the hand-written
script of tests/search_samples_helpers.py and a seeded random one), ``ka_policy_ce_soft`` against the float64 reference under
the update head's bound (MARGIN x e32, tests/update_head_helpers.py) and bit for bit against ``ka_policy_ce`` where the
contract says so, ``ka_sl_gather_visits`` against the numpy restatements, then the whole path: an arena round with a
visit-count search whose drained dataset is the restatement fed with the recorded plies, joins the game log's replay, and
trains an ``SLTrainer`` with ``visit_targets=True``."""
import numpy as np
import pytest
import torch

import mate3_helpers as M3
import mate_search_helpers as MH
import search_samples_helpers as S
import update_head_helpers as H
from keisei_amd import _lib
from keisei_amd.sl import DeviceSLDataset
from keisei_amd.sl.dataset import NUM_ACTIONS
from keisei_amd.sl.device_dataset import mirror_action, mirror_visit_words, sl_mirror_draw, visit_weights
from keisei_amd.sl.prepare import dataset_from_recorded_games
from keisei_amd.sl.trainer import SLConfig, SLTrainer
from keisei_amd.training import MatchArena, MateControls, MctsControls
from keisei_amd.training import search_samples as ss
from keisei_amd.training.model_registry import build_model
from test_hip_lookahead_replies import _group

pytestmark = pytest.mark.gpu
DEV = "cuda"
MP = dict(num_blocks=2, channels=32, se_reduction=8, global_pool_channels=16, policy_channels=8,
          value_fc_size=32, score_fc_size=16, obs_channels=50)


def st():
    return _lib.stream_ptr()


def dev(x):
    return (torch.from_numpy(np.ascontiguousarray(x)) if isinstance(x, np.ndarray) else x.contiguous()).to(DEV)


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------ ka_search_sample_step
def run_script(script, W, plies, R=S.R, spoil=None):
    """Every ply of ``script`` through the kernel and the restatement; both stores compared after every launch."""
    n = len(script)
    rows_d = torch.zeros(n * R, ss.ROW_WORDS, dtype=torch.int32, device=DEV)
    meta_d = torch.zeros(n * ss.META_WORDS + 1, dtype=torch.int32, device=DEV)
    rows_h, meta_h, err_h = np.zeros((n, R, ss.ROW_WORDS), np.uint32), np.zeros((n, ss.META_WORDS), np.int32), 0
    for t in range(plies):
        p = S.script_ply(t, W, script)
        if spoil is not None:
            spoil(t, p)
        _lib.call("ka_search_sample_step", dev(p["obs"]), 4050, dev(p["players"]), dev(p["records"]), p["records"].shape[1],
                  dev(p["root_visits"]), W, dev(p["model_of"]), dev(p["actions"]), dev(p["material"]), dev(p["rewards"]),
                  dev(p["terminated"]), dev(p["truncated"]), rows_d, R, meta_d, meta_d.data_ptr() + 4 * n * ss.META_WORDS, n, st())
        err_h |= ss.search_sample_step_host(rows_h, meta_h, p["obs"], p["players"], p["records"], p["root_visits"],
                                            p["model_of"], p["actions"], p["material"], p["rewards"], p["terminated"],
                                            p["truncated"])
        got_meta = meta_d.cpu().numpy()
        assert np.array_equal(got_meta[:-1].reshape(n, -1), meta_h), (t, got_meta, meta_h)
        assert int(got_meta[-1]) == err_h, t
        got = rows_d.cpu().numpy().view(np.uint32).reshape(n, R, ss.ROW_WORDS)
        assert np.array_equal(got, rows_h), (t, np.argwhere(got != rows_h)[:8])
    return rows_h, meta_h, err_h


@pytest.mark.parametrize("W", (3, 8))
def test_sample_step_on_the_script(W):
    rows, meta, err = run_script(S.SCRIPT, W, S.T)
    want_rows, want_meta = S.expected_store(W)
    assert err == 0 and np.array_equal(rows, want_rows) and np.array_equal(meta, want_meta)


@pytest.mark.parametrize("W", (3, 8))
def test_sample_step_on_a_random_script(W):
    script = S.random_script(11 + W)
    rows, meta, err = run_script(script, W, len(script[0]))
    assert err == 0 and meta[:, 2].any() and meta[:, 4].any() and (meta[:, 0] == S.R).any()


def test_sample_step_flags_an_unpackable_observation():
    def spoil(t, p):
        if t == 1:
            p["obs"][1, 81 * 7 + 4], p["obs"][1, 81 * 7 + 9] = 1.0, 2.0     # two patterns in one channel of an env that writes
        if t == 0:
            p["obs"][3, 81 * 7 + 4], p["obs"][3, 81 * 7 + 9] = 1.0, 2.0     # an inactive env: its observation is never packed
    _, _, err = run_script(S.SCRIPT, 3, 3, spoil=spoil)
    assert err == ss.ERR_UNPACKABLE


# ------------------------------------------------------------------------------------------------ ka_policy_ce_soft
def held(kernel, case, got, ref, e32):
    worst = 0.0
    for k in e32:
        x = H.excess(got[k], ref[k], e32[k])
        print(f"ratio {kernel} {case} {k} {x:.3f} (e32 {e32[k]:.3e})")
        worst = max(worst, x)
    assert worst <= H.MARGIN, (kernel, case, worst)


def run_soft(logits, actions, weights, w_policy, gscale=None, with_dl=True):
    B, A = logits.shape
    K = actions.shape[1]
    dl = torch.full((B, A), 7.0, device=DEV) if with_dl else None
    rl = torch.full((B,), 7.0, device=DEV)
    flags = torch.zeros(2, dtype=torch.int32, device=DEV)
    gs = None if gscale is None else torch.tensor([gscale], device=DEV)
    _lib.call("ka_policy_ce_soft", dev(logits), dev(actions), dev(weights), K, dl, rl, flags, gs, w_policy, B, A, st())
    return rl.cpu(), (dl.cpu() if with_dl else None), flags.cpu().tolist()


@pytest.mark.parametrize("K", (1, 8))
@pytest.mark.parametrize("A", H.POLICY_A)
def test_policy_ce_soft_against_fp64(A, K):
    logits, actions, weights = S.soft_case(A, K)
    B, w = S.SOFT_B, H.W.lambda_policy / S.SOFT_B
    ref, e32 = H.with_e32(lambda dt: S.soft_ce_ref(logits, actions, weights, w, dt))
    rl, dl, flags = run_soft(logits, actions, weights, w)
    assert flags == [0, 0]
    held("policy_ce_soft", f"A{A}-K{K}", {"rowloss": rl, "dlogits": dl}, ref, e32)
    # bit for bit: the rows with one slot of weight 1 are ka_policy_ce's
    targets = torch.zeros(B, dtype=torch.int64)
    for b in S.ONE_SLOT:
        assert float(weights[b, b % K]) == 1.0 and int((weights[b] > 0).sum()) == 1
        targets[b] = int(actions[b, b % K])
    dl1, rl1, f1 = torch.empty(B, A, device=DEV), torch.empty(B, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
    _lib.call("ka_policy_ce", dev(logits), dev(targets), None, dl1, rl1, f1, None, w, B, A, st())
    for b in S.ONE_SLOT:
        assert same_bits(rl[b:b + 1], rl1.cpu()[b:b + 1]) and same_bits(dl[b], dl1.cpu()[b]), (A, K, b)
    # a power-of-two loss scale scales the gradient exactly and leaves the row losses
    rl2, dl2, _ = run_soft(logits, actions, weights, w, gscale=H.GSCALE)
    assert same_bits(rl2, rl) and same_bits(dl2, dl * H.GSCALE)
    ka, dl3, _ = run_soft(logits, actions, weights, w, gscale=H.GSCALE, with_dl=False)
    assert dl3 is None and same_bits(ka, rl)


FLAG_CASES = {
    "nan_logit": (0, lambda lg, a, w: lg.__setitem__((2, 3), float("nan"))),
    "action_above": (1, lambda lg, a, w: a.__setitem__((2, 0), lg.shape[1])),
    "action_below": (1, lambda lg, a, w: a.__setitem__((2, 0), -1)),
    "negative_weight": (1, lambda lg, a, w: w.__setitem__((2, 1), -0.25)),
    "infinite_weight": (1, lambda lg, a, w: w.__setitem__((2, 1), float("inf"))),
    "nan_weight": (1, lambda lg, a, w: w.__setitem__((2, 1), float("nan"))),
    "no_used_slot": (1, lambda lg, a, w: w.__setitem__(2, 0.0)),
}


@pytest.mark.parametrize("name", FLAG_CASES)
def test_policy_ce_soft_flags(name):
    which, spoil = FLAG_CASES[name]
    logits, actions, weights = (x.clone() for x in S.soft_case(257, 8))
    w = 1.0 / S.SOFT_B
    rl0, dl0, flags0 = run_soft(logits, actions, weights, w)
    spoil(logits, actions, weights)
    rl, dl, flags = run_soft(logits, actions, weights, w)
    assert flags0 == [0, 0] and flags[which] == 1 and flags[1 - which] == 0, (name, flags)
    keep = [b for b in range(S.SOFT_B) if b != 2]
    assert same_bits(rl[keep], rl0[keep]) and same_bits(dl[keep], dl0[keep])          # the other rows are what they were
    if which == 1:
        assert float(rl[2]) == 0.0 and not dl[2].any()


def test_policy_ce_soft_refuses_a_bad_slot_count():
    logits, actions, weights = S.soft_case(33, 8)
    for K in (0, 65):
        with pytest.raises(_lib.KeiseiHipError, match="policy_ce_soft: K"):
            _lib.call("ka_policy_ce_soft", dev(logits), dev(actions), dev(weights), K, None, torch.empty(16, device=DEV),
                      torch.zeros(2, dtype=torch.int32, device=DEV), None, 1.0, 16, 33, st())


# ------------------------------------------------------------------------------------------------ ka_sl_gather_visits
def visit_table(n=20, seed=3):
    g = np.random.default_rng(seed)
    v = g.integers(0, 65, (n, 8)) * (g.random((n, 8)) < 0.6)
    v[:, 0] = np.maximum(v[:, 0], 1)
    v[4, 1:] = 0
    return ss.visit_words(g.integers(0, NUM_ACTIONS, (n, 8)), v)


@pytest.mark.parametrize("mode", (0, 1, 2))
def test_gather_visits_equals_the_host_restatement(mode):
    words, n, seed, epoch = visit_table(), 20, 20260, 3
    idx = np.array([19, 0, 4, 4, 25, 7, -1], np.int64)                     # B = 7: a repeat and two indices outside
    inside = (idx >= 0) & (idx < n)
    reflect = {0: np.zeros(7, bool), 1: np.ones(7, bool), 2: sl_mirror_draw(seed, epoch, idx)}[mode] & inside
    if mode == 2:
        assert reflect.any() and not reflect[inside].all()
    acts = torch.full((7, 8), 99, dtype=torch.int32, device=DEV)
    wts = torch.full((7, 8), 99.0, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.call("ka_sl_gather_visits", dev(words.view(np.int32)), n, dev(idx), 7, mode, seed, epoch, acts, wts, flag, st())
    rows = np.where(inside[:, None], words[np.clip(idx, 0, n - 1)], 0).astype(np.uint32)
    rows = np.where(reflect[:, None], mirror_visit_words(rows), rows)
    want_a, _ = ss.unpack_visit_words(rows)
    assert np.array_equal(acts.cpu().numpy(), want_a)
    assert wts.cpu().numpy().tobytes() == visit_weights(rows).tobytes()
    assert (want_a[~inside] == -1).all() and not visit_weights(rows)[~inside].any() and int(flag.item()) == 0
    if mode == 2:                                                          # exactly the drawn rows differ from the plain ones
        plain, _ = ss.unpack_visit_words(np.where(inside[:, None], words[np.clip(idx, 0, n - 1)], 0))
        assert np.array_equal((acts.cpu().numpy() != plain).any(1), reflect)


def test_append_packed_validates_on_the_device_and_views_carry_the_rows():
    g = np.random.default_rng(5)
    packed = np.zeros((6, 204), np.int32)
    packed[:, 200], packed[:, 201] = g.integers(0, NUM_ACTIONS, 6), g.integers(0, 3, 6)
    words, info = visit_table(6).view(np.int32), g.integers(0, 100, (6, 4)).astype(np.int32)
    ds = DeviceSLDataset()
    ds.append_packed(dev(packed), dev(words), dev(info))
    ds.append_packed(dev(packed[:2]), dev(words[:2]))
    ds.check()
    assert len(ds) == 8 and np.array_equal(ds.visits.cpu().numpy(), np.concatenate([words, words[:2]]))
    assert np.array_equal(ds.info.cpu().numpy()[:6], info) and not ds.info.cpu().numpy()[6:].any()
    part = ds.view(2, 5)
    assert torch.equal(part.visits, ds.visits[2:5]) and torch.equal(part.info, ds.info[2:5]) and part.visits.data_ptr() == ds.visits[2:].data_ptr()
    got = part.gather(torch.tensor([0, 2], device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV), visit_targets=True)
    assert got["visit_weights"].cpu().numpy().tobytes() == visit_weights(words[[2, 4]].view(np.uint32)).tobytes()
    with pytest.raises(ValueError, match="holds visit rows"):
        ds.append_packed(dev(packed))
    plain = DeviceSLDataset()
    plain.append_packed(dev(packed))
    plain.check()
    assert plain.visits is None and plain.info is None and len(plain) == 6
    with pytest.raises(ValueError, match="without visit rows"):
        plain.append_packed(dev(packed), dev(words))
    with pytest.raises(ValueError, match="needs a dataset with visit rows"):
        plain.gather(torch.tensor([0], device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV), visit_targets=True)
    # growth past the first allocation keeps the side rows beside their positions
    big = DeviceSLDataset()
    for _ in range(260):
        big.append_packed(dev(packed), dev(words), dev(info))
    big.check()
    assert len(big) == 1560 and torch.equal(big.visits[-6:].cpu(), torch.from_numpy(words)) and torch.equal(big.info[:6].cpu(), torch.from_numpy(info))
    # each fault is flagged at its row
    def spoiled(row, col, value, visits=words):
        p, v = packed.copy(), visits.copy()
        (p if col >= 0 else v)[row, col if col >= 0 else -col - 1] = value
        bad = DeviceSLDataset()
        bad.append_packed(dev(packed[:3]), dev(words[:3]))
        bad.append_packed(dev(p), dev(v))
        return bad
    for row, col, value in ((1, 200, NUM_ACTIONS), (2, 200, -1), (3, 201, 3), (0, 201, -1), (5, -1, (1 << 16) | NUM_ACTIONS)):
        with pytest.raises(ValueError, match=f"at index {3 + row}:"):
            spoiled(row, col, value).check()
    empty = words.copy()
    empty[4] = 77                                                          # actions without visits: no used slot
    with pytest.raises(ValueError, match="at index 7:"):
        spoiled(0, 200, 0, visits=empty).check()


# ------------------------------------------------------------------------------------------------ through the arena
N, PER, CTL = 8, 4, [MctsControls(width=3, simulations=4)] * 2
PAIRINGS = [(0, 1), (1, 0), (1, 1)]


def host_store(records, R, W):
    rows, meta, err = np.zeros((N, R, ss.ROW_WORDS), np.uint32), np.zeros((N, ss.META_WORDS), np.int32), 0
    for rec in records:
        err |= ss.search_sample_step_host(rows, meta, rec["obs"], rec["pre_players"], rec["mcts_records"][0],
                                          rec["mcts_root_visits"][1], rec["model_of"], rec["actions"], rec["material_balance"],
                                          rec["rewards"], rec["terminated"], rec["truncated"])
    return rows, meta, err


@pytest.fixture(scope="module")
def truncated_round():
    """One recorded round from the standard start with max_ply 5: every game ends by truncation inside the round."""
    arena = MatchArena(_group(), N, PER, 5, sync_every=2, graph=False, seed=29, record=True, game_log=256, mcts=CTL,
                       search_samples=32)
    results, stats = arena.run_round(PAIRINGS, games_per_match=4)
    records = arena.record
    dataset, drained = arena.search_samples.drain()
    return arena, results, stats, records, dataset, drained


def test_the_drained_dataset_is_the_restatement_fed_with_the_recorded_plies(truncated_round):
    arena, results, stats, records, ds, drained = truncated_round
    games = [g for r in results for g in r.recorded_games]
    assert games and all(g.truncated and g.winner == 2 for g in games) and stats.games_dropped == 0
    assert all("material_balance" in rec for rec in records)
    rows, meta, err = host_store(records, 32, 3)
    assert err == 0 and not meta[:, 2].any()
    want = np.concatenate([rows[e, :meta[e, 1]] for e in range(N)])
    assert (drained.written, drained.labelled, drained.discarded, drained.dropped) == (
        int(meta[:, 0].sum()), len(want), int((meta[:, 0] - meta[:, 1]).sum()), 0)
    assert len(ds) == len(want) >= len(games) and stats.mcts.searched >= len(want)
    assert np.array_equal(ds.packed.cpu().numpy().view(np.uint32), want[:, :204])
    assert np.array_equal(ds.visits.cpu().numpy().view(np.uint32), want[:, 204:212])
    assert np.array_equal(ds.info.cpu().numpy().view(np.uint32), want[:, 212:])
    assert (want[:, 201] == 1).all()                                       # every game was a draw by truncation
    # each row's visits are the root visits of its ply: walk the recorded plies again, env by env
    at = {}
    moves, game = np.zeros(N, int), np.zeros(N, int)
    for rec in records:
        cand, visits, _ = rec["mcts_root_visits"]
        for e in range(N):
            at[(e, int(game[e]), int(moves[e]))] = (cand[e].numpy(), visits[e].numpy(), int(rec["actions"][e]))
            done = bool(rec["terminated"][e]) or bool(rec["truncated"][e])
            moves[e], game[e] = (0, game[e] + 1) if done else (moves[e] + 1, game[e])
    info = ds.info.cpu().numpy()
    a, v = ss.unpack_visit_words(ds.visits.cpu().numpy())
    for i in range(len(ds)):
        cand, visits, played = at[(int(info[i, 2]), int(info[i, 3]), int(info[i, 1]))]
        used = visits > 0
        assert np.array_equal(v[i, :3], visits) and np.array_equal(a[i, :3][used], cand[used]) and not v[i, 3:].any()
        assert int(ds.packed[i, 200]) == played and visits.sum() >= 4
    # the store is empty, the counters of the open games go on
    m2, e2 = arena.search_samples.meta()
    assert e2 == 0 and not m2[:, :3].any() and np.array_equal(m2[:, 3:].numpy(), meta[:, 3:])
    again, stats2 = arena.search_samples.drain(into=ds)
    assert again is ds and stats2 == ss.SearchSampleStats() and len(ds) == len(want)


def test_the_rows_join_the_replay_of_the_logged_games(truncated_round):
    arena, results, stats, records, ds, drained = truncated_round
    games = [g for r in results for g in r.recorded_games if g.is_standard_start and len(g.actions)]
    replay, meta = dataset_from_recorded_games(games, max_moves=5)
    assert len(replay) == sum(len(g.actions) for g in games)
    offset, first = {}, 0
    for g in games:
        offset[(g.env, g.game_number)] = (first, len(g.actions))
        first += len(g.actions)
    info, mine, theirs = ds.info.cpu().numpy(), ds.packed.cpu().numpy(), replay.packed.cpu().numpy()
    joined = 0
    for i in range(len(ds)):
        key = (int(info[i, 2]), int(info[i, 3]))
        if key in offset:
            lo, n = offset[key]
            assert int(info[i, 1]) < n
            assert np.array_equal(mine[i], theirs[lo + int(info[i, 1])]), (i, key)
            joined += 1
    assert joined >= len(games)


def test_decisive_games_label_their_rows_for_the_mover():
    """Games from the mate-in-one pool and the mate-in-three pool, model 0 alone looking for mates (three deep): a mate in one
    is a game of one row, won by its mover; a mate in three is check, forced evasion, mate -- the defender's row is a loss."""
    deep = [MateControls(*M3.POOL_CAPS[:1], 0, *M3.POOL_CAPS[1:]), MateControls.OFF]
    arena = MatchArena(_group(), N, PER, 40, sync_every=2, graph=True, seed=17, game_log=256, start_pool_capacity=32,
                       mcts=[MctsControls(1, 2, 1.25)] * 2, mate=deep, search_samples=256)
    arena.env.set_start_sfens(MH.pool_sfens() + M3.pool_sfens(), seed=5)
    results, stats = arena.run_round([(0, 1), (1, 0)], games_per_match=8)
    ds, drained = arena.search_samples.drain()
    winner = {(g.env, g.game_number): g.winner for r in results for g in r.recorded_games}
    assert drained.dropped == 0 and drained.labelled == len(ds) > 0 and stats.games_dropped == 0
    info, value = ds.info.cpu().numpy(), ds.packed[:, 201].cpu().numpy()
    seen, matched = set(), 0
    for i in range(len(ds)):
        key = (int(info[i, 2]), int(info[i, 3]))
        assert value[i] in (0, 1, 2)
        if key in winner:
            w, mover = winner[key], (int(info[i, 0]) >> 16) & 1
            assert int(value[i]) == (1 if w == 2 else (0 if w == mover else 2)), (i, key, w, mover)
            seen.add(int(value[i]))
            matched += 1
    assert matched >= 8 and {0, 2} <= seen


def test_graph_equals_eager():
    out = []
    for graph in (False, True):
        arena = MatchArena(_group(), N, PER, 6, sync_every=2, graph=graph, seed=23, game_log=256, mcts=CTL, search_samples=32)
        results, stats = arena.run_round(PAIRINGS, games_per_match=4)
        ds, drained = arena.search_samples.drain()
        assert (arena._graph is not None) == graph and len(ds) > 0 and drained.dropped == 0
        out.append((ds, drained))
    (a, sa), (b, sb) = out
    assert sa == sb and torch.equal(a.packed, b.packed) and torch.equal(a.visits, b.visits) and torch.equal(a.info, b.info)


def test_the_ply_is_unchanged_when_off(monkeypatch):
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: names.append(name) or real(name, *a))
    seqs = []
    for kw in ({}, dict(search_samples=0), dict(search_samples=8)):
        arena = MatchArena(_group(), N, PER, 6, sync_every=2, graph=False, seed=23, mcts=CTL, **kw)
        del names[:]
        arena.run_round(PAIRINGS[:1], games_per_match=4)
        seqs.append(list(names))
        assert (arena.search_samples is None) == (not kw.get("search_samples")) and arena.ply.search_samples is arena.search_samples
    assert seqs[0] == seqs[1] and "ka_search_sample_step" not in seqs[0]
    assert [n for n in seqs[2] if n != "ka_search_sample_step"] == seqs[0]
    assert seqs[2].count("ka_search_sample_step") == seqs[2].count("ka_arena_referee")
    i = seqs[2].index("ka_search_sample_step")
    assert seqs[2][i - 1] == "ka_shogi_env_step" and seqs[2][i + 1] == "ka_arena_referee"
    with pytest.raises(ValueError, match="search_samples needs mcts="):
        MatchArena(_group(), N, PER, 6, graph=False, search_samples=8)


# ------------------------------------------------------------------------------------------------ through the trainer
def dataset_with(packed, visits):
    ds = DeviceSLDataset()
    ds.append_packed(packed.contiguous(), visits.contiguous())
    ds.check()
    return ds


def fresh_trainer(sd0, ds, **config):
    model = build_model("se_resnet", MP)
    model.load_state_dict(sd0)
    model.to(DEV)
    return model, SLTrainer(model, SLConfig(data_dir="/nonexistent/never/read", batch_size=24, total_epochs=5, **config), dataset=ds)


@pytest.fixture(scope="module")
def sampled(truncated_round):
    ds = truncated_round[4]
    n = min(len(ds), 64)
    assert n >= 40
    torch.manual_seed(9)
    sd0 = {k: v.clone() for k, v in build_model("se_resnet", MP).state_dict().items()}
    return ds.packed[:n].clone(), ds.visits[:n].clone(), sd0, torch.from_numpy(np.random.default_rng(8).permutation(n))


def test_visits_on_the_played_move_alone_train_as_the_one_hot_epoch(sampled):
    packed, _, sd0, order = sampled
    visits = torch.zeros(len(packed), 8, dtype=torch.int32, device=DEV)
    visits[:, 2] = packed[:, 200] | (5 << 16)                              # five visits, all on the move played
    states = []
    for on in (True, False):
        ds = dataset_with(packed, visits)
        model, trainer = fresh_trainer(sd0, ds, visit_targets=on)
        trainer._order_override = order
        met = trainer.train_epoch()
        states.append((met, {k: v.detach().cpu().clone() for k, v in model.state_dict().items()}))
    assert states[0][0] == states[1][0]
    for k, v in states[0][1].items():
        assert torch.equal(v, states[1][1][k]), k
    assert any(not torch.equal(v, sd0[k]) for k, v in states[0][1].items() if v.is_floating_point())


def test_a_spread_visit_epoch_trains_on_the_soft_loss(sampled, monkeypatch):
    packed, visits, sd0, order = sampled
    ds = dataset_with(packed, visits)
    assert int(((visits >> 16) > 0).sum(1).max()) > 1
    calls, soft = [], []
    real = _lib.call

    def spy(name, *a):
        calls.append(name)
        if name == "ka_policy_ce_soft":
            soft.append((a[0].clone(), a[1].clone(), a[2].clone(), a[5]))
        return real(name, *a)
    monkeypatch.setattr(_lib, "call", spy)
    model, trainer = fresh_trainer(sd0, ds, visit_targets=True)
    trainer._order_override = order
    met = trainer.train_epoch()
    batches = -(-len(packed) // 24)
    assert calls.count("ka_policy_ce_soft") == batches == len(soft) and "ka_policy_ce" not in calls
    assert calls.count("ka_sl_gather_visits") == batches
    means = []
    words = visits.cpu().numpy().view(np.uint32)
    for k, (logits, actions, weights, rowloss) in enumerate(soft):
        idx = order[24 * k:24 * (k + 1)].numpy()
        want_a, _ = ss.unpack_visit_words(words[idx])
        assert np.array_equal(actions.cpu().numpy(), want_a) and weights.cpu().numpy().tobytes() == visit_weights(words[idx]).tobytes()
        ref, e32 = H.with_e32(lambda dt: {"rowloss": S.soft_ce_ref(logits.cpu(), actions.cpu(), weights.cpu(), 1.0, dt)["rowloss"]})
        held("trainer policy_ce_soft", f"batch{k}", {"rowloss": rowloss.cpu()}, ref, e32)
        means.append(float(rowloss.double().mean()))
    # the batch mean is an fp32 sum of at most 24 non-negative terms and one division, the epoch's a sum of three such means
    want = float(np.mean(means))
    assert abs(met["policy_loss"] - want) <= 32 * 2.0 ** -24 * want, (met["policy_loss"], want)
    keys = trainer.evaluate(ds)
    assert set(keys) == {"policy_loss", "value_loss", "score_loss", "policy_top1", "policy_topk", "value_accuracy", "positions"}
    assert keys["positions"] == len(packed)


def test_a_mirror_augmented_visit_epoch_reflects_the_drawn_rows(sampled, monkeypatch):
    packed, visits, sd0, order = sampled
    ds = dataset_with(packed, visits)
    soft = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (soft.append(a[1].clone()) if name == "ka_policy_ce_soft" else None) or real(name, *a))
    model, trainer = fresh_trainer(sd0, ds, visit_targets=True, mirror_augment=True, mirror_seed=20260)
    trainer._order_override = order
    met = trainer.train_epoch()
    assert np.isfinite(met["policy_loss"]) and met["policy_loss"] > 0
    words = visits.cpu().numpy().view(np.uint32)
    drawn = sl_mirror_draw(20260, 0, np.arange(len(packed)))
    assert drawn.any() and not drawn.all()
    for k, actions in enumerate(soft):
        idx = order[24 * k:24 * (k + 1)].numpy()
        rows = np.where(drawn[idx][:, None], mirror_visit_words(words[idx]), words[idx])
        want_a, _ = ss.unpack_visit_words(rows)
        assert np.array_equal(actions.cpu().numpy(), want_a)
        plain, _ = ss.unpack_visit_words(words[idx])
        used = plain >= 0
        assert np.array_equal(want_a[drawn[idx]][used[drawn[idx]]], mirror_action(plain[drawn[idx]][used[drawn[idx]]]))


def test_visit_targets_refuses_a_dataset_without_visit_rows(sampled):
    packed, _, sd0, _ = sampled
    plain = DeviceSLDataset()
    plain.append_packed(packed.contiguous())
    with pytest.raises(ValueError, match="needs a dataset with visit rows"):
        fresh_trainer(sd0, plain, visit_targets=True)
