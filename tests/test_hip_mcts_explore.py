"""The exploration of the visit-count search on the device: ka_mcts_root_noise alone on poisoned synthetic records,
ka_mcts_advance_explore against ka_mcts_advance (off) and against visit_choice_host (on) on the synthetic worlds of
tests/mcts_helpers.py, MctsSearch.step on a real env, and MatchArena(mcts=, mcts_explore=) game by game.

The fixed seeds satisfy the margin condition that tests/test_mcts_explore_cpu.py asserts: no accept test of their Dirichlet
draws is decided by less than 1e-9, so the device's fp64 log / cos / exp cannot send a draw down another branch.  Env counts:
the noise kernel runs one lane per (env, slot) with eight lanes per env, so a wave holds eight envs and a block thirty-two."""
import gc

import numpy as np
import pytest
import torch

import mcts_explore_helpers as XH
import mcts_helpers as H
from keisei_amd import _lib
from keisei_amd.shogi_gym import ACTION_SPACE, VecEnv
from keisei_amd.training import (MatchArena, MctsControls, MctsExploration, MctsSearch, explore_table, mcts_backup_select,
                                 mcts_table, root_noise_host, visit_choice_host)
from keisei_amd.training import search_samples as ss
from keisei_amd.training.lookahead import (FLAG_ACTIVE, FLAG_CHANGED, FLAG_WON, REC_ACTION, REC_CAND, REC_FLAGS, REC_NCAND,
                                           REC_SLOT)
from keisei_amd.training.mcts_explore import FLAG_DIVERGED, FLAG_SAMPLED, explore_controls
from keisei_amd.training.tree_search import FLAG_DEEPENED
from test_hip_lookahead_replies import _games, _group, _key, _lowest_legal, _stream

pytestmark = pytest.mark.gpu
DEV = "cuda"
ULP = 2.0 ** -23
_HIP_ERROR = []


@pytest.fixture(autouse=True)
def _release_device_objects():
    """Arenas own captured graphs and pinned buffers: collect them with the device idle, not inside a later test's capture.
    A HIP error ends the module: once a synchronise has raised, no later test of it touches the device."""
    if _HIP_ERROR:
        pytest.fail("an earlier test of this module met a HIP error: nothing more of it runs on the device")
    yield
    gc.collect()
    try:
        torch.cuda.synchronize()
    except Exception:
        _HIP_ERROR.append(True)
        raise
    gc.collect()


def _dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dtype is None else t.to(dtype)


def _xtable(controls, K=2):
    return _dev(explore_table(controls, K))


def _seed(value):
    return torch.tensor([value], dtype=torch.int64, device=DEV)


# ------------------------------------------------------------------ 1. the noise kernel alone
@pytest.mark.parametrize("W", XH.NOISE_W)
@pytest.mark.parametrize("B", XH.NOISE_B)
def test_root_noise_is_the_restatement_and_writes_nothing_else(B, W):
    """p' within one fp32 ulp of 1 (both sides round one fp64 value in [0, 1] whose two computations agree to the last bits),
    eta to 1e-12, every word the kernel has no business with still poison, the counter the number of noised rows."""
    c = XH.noise_case(B, W)
    words, pad = c["rec"].shape[1], 64
    rec = torch.full((pad + B * words + pad,), int(XH.POISON), dtype=torch.int32, device=DEV)
    rec[pad:pad + B * words] = _dev(c["rec"]).reshape(-1)
    raw = torch.full((pad + B * W + pad,), int(XH.POISON), dtype=torch.int32, device=DEV)
    eta = torch.full((pad + B * W + pad,), -7.0, dtype=torch.float64, device=DEV)
    stats = torch.tensor([5, 11, 13, 17], dtype=torch.int32, device=DEV)
    _lib.call("ka_mcts_root_noise", rec.data_ptr() + 4 * pad, W, _xtable(c["ctl"]), _dev(c["model_of"]), 2, _seed(c["seed"]),
              raw.data_ptr() + 4 * pad, eta.data_ptr() + 8 * pad, stats, B, _stream())
    torch.cuda.synchronize()
    before = c["rec"]
    pri = slice(REC_CAND + W, REC_CAND + 2 * W)
    want, want_eta, margin = root_noise_host(c["seed"], before[:, pri].view(np.float32), c["n_cand"], c["active"], c["ctl"],
                                             c["model_of"])
    assert (margin >= XH.MARGIN).all()
    noised = c["active"] & (c["model_of"] == 0)
    got = rec.cpu().numpy()
    got_rec = got[pad:pad + B * words].reshape(B, words)
    poison = int(XH.POISON)
    assert (got[:pad] == poison).all() and (got[pad + B * words:] == poison).all()
    other = np.ones(words, bool)
    other[pri] = False
    assert np.array_equal(got_rec[:, other], before[:, other])             # flags, counts, candidates, q: as they were
    used = np.arange(W)[None, :] < c["n_cand"][:, None]
    write = noised[:, None] & used
    assert np.array_equal(got_rec[:, pri][~write], before[:, pri][~write])  # slots >= n and the rows not noised: to the bit
    got_p = got_rec[:, pri].view(np.float32)
    diff = np.abs(got_p[write].astype(np.float64) - want[write].astype(np.float64))
    print(f"B {B} W {W}: noised rows {int(noised.sum())}, max |p' - ref| {diff.max():.3e}, cells off by an ulp {int((diff > 0).sum())}")
    assert (diff <= ULP).all()
    raw_h, eta_h = raw.cpu().numpy(), eta.cpu().numpy()
    assert (raw_h[:pad] == poison).all() and (raw_h[pad + B * W:] == poison).all()
    assert (eta_h[:pad] == -7.0).all() and (eta_h[pad + B * W:] == -7.0).all()
    raw_h, eta_h = raw_h[pad:pad + B * W].reshape(B, W), eta_h[pad:pad + B * W].reshape(B, W)
    assert (raw_h[~noised] == poison).all() and (eta_h[~noised] == -7.0).all()
    assert np.array_equal(raw_h[write], before[:, pri][write]) and not raw_h[noised[:, None] & ~used].any()
    print(f"           max |eta - ref| {np.abs(eta_h[noised] - want_eta[noised]).max():.3e}")
    assert (np.abs(eta_h[noised] - want_eta[noised]) <= 1e-12).all() and not eta_h[noised[:, None] & ~used].any()
    assert stats.cpu().tolist() == [5 + int(noised.sum()), 11, 13, 17]


# ------------------------------------------------------------------ 2., 3. the advance
GAME_PLY = 6                                                  # the made-up game ply of every row of a synthetic world


def _advance(world, xtable, seed):
    """A synthetic world through ka_mcts_advance (``xtable`` None) or ka_mcts_advance_explore, as tests/test_hip_mcts.py walks
    it.  Returns per simulation ``(records, tree words, parent_row, active)`` and the buffers behind the last launch."""
    W, E, B = world["W"], world["E"], world["B"]
    P = E * B * W
    pool_vl, pool_rw = _dev(world["vl"].reshape(P, 3), torch.float32), _dev(world["rewards"].reshape(P), torch.float32)
    pool_term, pool_trunc = _dev(world["done"].reshape(P), torch.bool), torch.zeros(P, dtype=torch.bool, device=DEV)
    rec = torch.zeros(E, B, _lib.query("ka_mcts_words", 0, W, E), dtype=torch.int32, device=DEV)
    tree = torch.full((B, _lib.query("ka_mcts_words", 1, W, E)), -5, dtype=torch.int32, device=DEV)
    step_err = torch.zeros(E, 2, dtype=torch.int64, device=DEV)
    buf = dict(actions=_dev(world["sampled"], torch.int64), pv=torch.full((B, E), -9, dtype=torch.int32, device=DEV),
               root_visits=torch.full((B, W), -9, dtype=torch.int32, device=DEV),
               root_values=torch.full((B, W), -9.0, dtype=torch.float32, device=DEV),
               counters=torch.zeros(7, dtype=torch.int32, device=DEV), xstats=torch.zeros(4, dtype=torch.int32, device=DEV))
    table = _dev(mcts_table(world["ctl"], 2))
    model_of = _dev(world["model_of"], torch.int32)
    parent_row = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    active = torch.zeros(B, dtype=torch.int32, device=DEV)
    plies = torch.full((B, 32), GAME_PLY, dtype=torch.int32, device=DEV)      # rows of 128 bytes, the ply at byte 100
    out = []

    def advance(t, rec_t):
        rec[t] = _dev(rec_t)
        args = (rec, tree, W, E, t, table, model_of, 2, pool_vl, pool_rw, pool_term, pool_trunc, step_err, buf["actions"],
                parent_row, active, buf["pv"], buf["root_visits"], buf["root_values"], buf["counters"],
                buf["counters"].data_ptr() + 24)
        if xtable is None:
            _lib.call("ka_mcts_advance", *args, B, _stream())
        else:
            _lib.call("ka_mcts_advance_explore", *args, xtable, seed, plies.data_ptr() + 100, 128, buf["xstats"], B, _stream())
        torch.cuda.synchronize()
        out.append((rec.cpu(), tree.cpu(), parent_row.cpu(), active.cpu()))
        return out[-1][3].numpy()

    H.walk(world, advance)
    return out, {k: v.cpu() for k, v in buf.items()}


@pytest.mark.parametrize("W,E", H.SHAPES)
def test_advance_explore_with_every_row_off_is_advance_bit_for_bit(W, E):
    world = H.make_world(W, E, H.SEEDS[W, E])
    plain, pbuf = _advance(world, None, None)
    off, obuf = _advance(world, _xtable(None), _seed(41))
    for t, (a, b) in enumerate(zip(plain, off)):              # records, tree, parent_row and active after every simulation
        assert all(torch.equal(x, y) for x, y in zip(a, b)), t
    for name in ("actions", "pv", "root_visits", "root_values", "counters"):
        assert torch.equal(pbuf[name], obuf[name]), name
    assert obuf["xstats"].tolist() == [0, 0, 0, 0] and int(pbuf["counters"][0]) == world["B"] - 1


@pytest.mark.parametrize("W,E", H.SHAPES)
def test_the_drawn_move_is_visit_choice_host_on_the_kernels_own_visits(W, E):
    """Model 0 draws (its sample_plies lies above the made-up game ply), model 1 does not (below it).  The tree does not
    depend on the choice: it is the restatement's, as tests/test_hip_mcts.py holds it."""
    world = H.make_world(W, E, H.SEEDS[W, E])
    B, seed = world["B"], 0x7EA5 + W
    ctl = [MctsExploration(0.0, 0.0, GAME_PLY + 1), MctsExploration(0.0, 0.0, GAME_PLY)]
    plain, pbuf = _advance(world, None, None)
    on, buf = _advance(world, _xtable(ctl), _seed(seed))
    rec, tree = on[-1][0], on[-1][1]
    rec0 = rec[0].numpy()
    root = (rec0[:, REC_FLAGS] & FLAG_ACTIVE) != 0
    visits = buf["root_visits"].numpy()
    assert torch.equal(buf["root_visits"], pbuf["root_visits"]) and torch.equal(buf["root_values"], pbuf["root_values"])
    assert torch.equal(tree, plain[-1][1])                    # the same tree as without exploration
    slot, sampled = visit_choice_host(seed, visits, rec0[:, REC_NCAND], np.full(B, GAME_PLY), ctl, world["model_of"])
    best = visit_choice_host(seed, visits, rec0[:, REC_NCAND], np.full(B, GAME_PLY), None, None)[0]
    assert np.array_equal(sampled[root], world["model_of"][root] == 0)
    assert np.array_equal(rec0[root, REC_SLOT], slot[root])
    chosen = rec0[np.arange(B), REC_CAND + np.where(root, slot, 0)]
    acts = buf["actions"].numpy()
    assert np.array_equal(acts, np.where(root, chosen, world["sampled"])) and np.array_equal(rec0[root, REC_ACTION], chosen[root])
    diverged = sampled & (slot != best)
    changed = chosen != world["sampled"]
    at = (0, np.arange(B), np.where(root, slot, 0))
    won = world["done"][at] & (world["rewards"][at] > 0)
    deepened = (plain[-1][0][0].numpy()[:, REC_FLAGS] & FLAG_DEEPENED) != 0   # best against the one-ply arg-max: unchanged
    flags = root * (FLAG_ACTIVE + FLAG_CHANGED * changed + FLAG_WON * won + FLAG_DEEPENED * deepened + FLAG_SAMPLED * sampled +
                    FLAG_DIVERGED * diverged)
    assert np.array_equal(rec0[:, REC_FLAGS], flags)
    pv, ppv = buf["pv"].numpy(), pbuf["pv"].numpy()
    assert np.array_equal(pv[root, 0], chosen[root]) and (pv[~root] == -1).all()
    same = root & ~diverged
    assert np.array_equal(pv[same], ppv[same])                # where best was played the line is the one of ka_mcts_advance
    c, x = buf["counters"].tolist(), buf["xstats"].tolist()
    assert c[:4] == [int(root.sum()), int((root & changed).sum()), int((root & won).sum()), int((root & deepened).sum())]
    assert c[4:] == pbuf["counters"].tolist()[4:]
    assert x == [0, int((root & sampled).sum()), int((root & diverged).sum()), 0]
    if E > 1:
        assert x[1] >= 10 and x[2] >= 1 and x[1] - x[2] >= 1 and int((root & ~sampled).sum()) >= 10
    # the tree is the restatement's: N, by and the fp32 sums exactly
    parent = tree[:, :E].numpy()
    want = mcts_backup_select(rec, world["done"], parent.T, world["ctl"], world["model_of"])
    part = lambda i: tree[:, E + i * E * W:E + (i + 1) * E * W].contiguous()  # noqa: E731
    assert np.array_equal(part(0).numpy(), want.N.reshape(B, -1)) and np.array_equal(part(3).numpy(), want.by.reshape(B, -1))
    assert np.array_equal(part(1).view(torch.float32).numpy(), want.S32.reshape(B, -1))
    assert np.array_equal(want.choice[root], best[root]) and np.array_equal(visits, want.visits)


# ------------------------------------------------------------------ 4. MctsSearch.step on a real env
def test_step_noises_the_root_of_a_real_env():
    n, W, E = XH.STEP_ENVS, XH.STEP_W, 4
    env = VecEnv(n, 40, "katago", "spatial", output="torch", check_actions=True)
    env.reset()
    grp = _group()
    model_of = torch.tensor([0, 1] * (n // 2), dtype=torch.int32, device=DEV)
    model_of[5] = -1
    logits = grp.forward(env.current().observations, model_of.clamp_min(0), check=False).policy_logits.reshape(n, ACTION_SPACE).clone()
    ms = MctsSearch(env, grp, W, E, explore=True)
    table = _dev(mcts_table([MctsControls(W, E, 1.25), MctsControls(W, E, 0.3)], 2))
    ctl = [MctsExploration(0.25, XH.STEP_ALPHA, 3), MctsExploration(0.5, XH.STEP_ALPHA, 0)]
    seed = _seed(XH.STEP_SEED)
    cur = env.current()
    actions = torch.tensor(_lowest_legal(cur.legal_mask_bits), dtype=torch.int64, device=DEV)
    plain = MctsSearch(env, grp, W, E)
    plain.clear()
    plain.step(logits, cur.legal_mask_bits, actions.clone(), model_of, table, _stream())
    ms.clear()
    ms.step(logits, cur.legal_mask_bits, actions, model_of, table, _stream(), explore_table=_xtable(ctl), seed=seed.data_ptr())
    torch.cuda.synchronize()
    stats = ms.read()
    rec, tree = ms.records().cpu(), {k: v.cpu().numpy() for k, v in ms.tree().items()}
    rec0 = rec[0].numpy()
    active = (rec0[:, REC_FLAGS] & FLAG_ACTIVE) != 0
    assert active.sum() == n - 1 and not active[5]
    pri = slice(REC_CAND + W, REC_CAND + 2 * W)
    raw, eta = (x.cpu().numpy() for x in ms.root_noise())
    # the fork's priors are those of a search without exploration, and the noise is the restatement's
    assert np.array_equal(raw[active], plain.records(0).cpu().numpy()[active][:, pri].view(np.float32))
    want, want_eta, margin = root_noise_host(XH.STEP_SEED, raw, rec0[:, REC_NCAND], active, ctl, model_of.cpu())
    assert (margin >= XH.MARGIN).all() and np.isfinite(margin[active]).all()
    got = rec0[:, pri].view(np.float32)
    assert (np.abs(got[active].astype(np.float64) - want[active].astype(np.float64)) <= ULP).all()
    assert (np.abs(eta[active] - want_eta[active]) <= 1e-12).all() and not eta[~active].any()
    assert (got[active] != raw[active]).any(1).all() and np.allclose(eta[active].sum(1), 1.0, atol=1e-12)
    # the tree's P at slice 0 is the noised record, and the whole tree is the restatement fed the kernel's own records
    assert np.array_equal(tree["P"][active, 0].view(np.int32), rec0[active][:, pri])
    done = (ms.terminated | ms.truncated).cpu().numpy().reshape(E, n, W)
    tree_want = mcts_backup_select(rec, done, tree["parent"].T, table.cpu().numpy(), model_of.cpu())
    assert np.array_equal(tree["N"][active], tree_want.N[active]) and np.array_equal(tree["by"][active], tree_want.by[active])
    assert np.array_equal(tree["S"][active], tree_want.S32[active])
    assert np.array_equal(tree["P"][active].astype(np.float64), tree_want.P[active])
    # the choice: the first plies of model 0 are drawn
    visits = ms.root_visits()[1].cpu().numpy()
    plies = env._state[:, 100:104].contiguous().view(torch.int32).reshape(-1).cpu().numpy()
    slot, sampled = visit_choice_host(XH.STEP_SEED, visits, rec0[:, REC_NCAND], plies, ctl, model_of.cpu())
    assert np.array_equal(rec0[active, REC_SLOT], slot[active])
    assert np.array_equal((rec0[:, REC_FLAGS] & FLAG_SAMPLED) != 0, sampled & active)
    assert (stats.searched, stats.noised, stats.sampled) == (n - 1, n - 1, int((sampled & active).sum())) and stats.sampled == n // 2
    env.step(actions)
    env.raise_if_refused()
    with pytest.raises(ValueError, match="built with explore=True"):
        plain.root_noise()
    with pytest.raises(ValueError, match="built with explore=True"):
        plain.step(logits, cur.legal_mask_bits, actions, model_of, table, _stream(), explore_table=_xtable(ctl), seed=seed.data_ptr())


# ------------------------------------------------------------------ 5. the arena
N, PER, MAX_PLY = 16, 8, 24
PAIRINGS = [(0, 1), (1, 0)]
CTL = [MctsControls(3, 4, 1.25)] * 2
XP = [MctsExploration(0.25, 0.3, 8), MctsExploration(0.25, 0.3, 0)]


def _arena(seed=23, graph=True, **kw):
    return MatchArena(_group(), N, PER, MAX_PLY, sync_every=2, graph=graph, seed=seed, game_log=512, mcts=CTL, **kw)


def _lines(results):
    """per (black, white): the distinct move lists of the games played from the first ply on by one pairing"""
    out = {}
    for r in results:
        for g in r.recorded_games:
            if not g.carried and g.is_standard_start:
                out.setdefault((g.black, g.white), set()).add(tuple(int(a) for a in g.actions))
    return out


def test_exploration_is_what_makes_the_games_differ():
    off, on, twin, other = _arena(), _arena(mcts_explore=XP), _arena(mcts_explore=XP), _arena(seed=24, mcts_explore=XP)
    r_off, s_off = off.run_round(PAIRINGS, games_per_match=16)
    lines = _lines(r_off)
    assert len(lines) >= 2 and sum(len(r.recorded_games) for r in r_off) >= 16
    assert all(len(v) == 1 for v in lines.values()), {k: len(v) for k, v in lines.items()}     # the gap: one game per colours
    assert (s_off.mcts.noised, s_off.mcts.sampled, s_off.mcts.diverged) == (0, 0, 0)
    r_on, s_on = on.run_round(PAIRINGS, games_per_match=16)
    assert max(len(v) for v in _lines(r_on).values()) > 1
    assert s_on.mcts.noised == s_on.mcts.searched > 100 and s_on.mcts.sampled > s_on.mcts.diverged >= 1
    r_twin, s_twin = twin.run_round(PAIRINGS, games_per_match=16)
    assert _games(r_twin) == _games(r_on) and _key(r_twin) == _key(r_on) and s_twin.mcts == s_on.mcts
    r_other, _ = other.run_round(PAIRINGS, games_per_match=16)
    assert _games(r_other) != _games(r_on)
    # off again under the same captured graph: the games of an arena that never explored, move for move
    graph, table = on._graph, on.ply.stages["mcts"].explore_table
    on.set_mcts_explore(None)
    r_back, s_back = on.run_round(PAIRINGS, games_per_match=16)
    assert on._graph is graph and on.ply.stages["mcts"].explore_table is table and not bool(table.any())
    assert _games(r_back) == _games(r_off) and _key(r_back) == _key(r_off) and s_back.mcts == s_off.mcts
    on.set_mcts_explore(XP)
    r_again, s_again = on.run_round(PAIRINGS, games_per_match=16)
    assert _games(r_again) == _games(r_on) and s_again.mcts == s_on.mcts
    with pytest.raises(ValueError, match="built without mcts_explore="):
        off.set_mcts_explore(XP)
    assert off.ply.stages["mcts"].explore_table is None and off.mcts._eta is None and off.mcts._counters.numel() == 7


def test_the_counters_and_the_samples_follow_the_recorded_plies():
    arena = _arena(seed=29, graph=False, record=True, mcts_explore=XP, search_samples=64)
    results, stats = arena.run_round(PAIRINGS, games_per_match=8)
    recs = arena.record
    _, _, plies_of = explore_controls(explore_table(XP, 2), [0, 1])
    searched = sampled = diverged = 0
    rows, meta, err = np.zeros((N, 64, ss.ROW_WORDS), np.uint32), np.zeros((N, ss.META_WORDS), np.int32), 0
    for rec in recs:
        rec0 = rec["mcts_records"][0].numpy()
        active = (rec0[:, REC_FLAGS] & FLAG_ACTIVE) != 0
        mo, ply = rec["model_of"].numpy(), rec["game_plies"].numpy()
        drawn = active & (ply < np.where(mo >= 0, plies_of[np.maximum(mo, 0)], 0))
        assert np.array_equal((rec0[:, REC_FLAGS] & FLAG_SAMPLED) != 0, drawn)
        cand, visits, _ = rec["mcts_root_visits"]
        slot, was = visit_choice_host(rec["seed"], visits, rec0[:, REC_NCAND], ply, XP, mo)
        assert np.array_equal(was & active, drawn) and np.array_equal(rec0[active, REC_SLOT], slot[active])
        assert np.array_equal(rec["actions"].numpy()[active], rec0[active, REC_ACTION])
        raw, eta = rec["mcts_root_noise"]
        assert np.allclose(eta.numpy()[active].sum(1), 1.0, atol=1e-12)
        W = 3
        assert np.array_equal(rec["mcts_tree"]["P"].numpy()[active, 0].view(np.int32), rec0[active][:, REC_CAND + W:REC_CAND + 2 * W])
        searched += int(active.sum())
        sampled += int(drawn.sum())
        diverged += int(((rec0[:, REC_FLAGS] & FLAG_DIVERGED) != 0).sum())
        err |= ss.search_sample_step_host(rows, meta, rec["obs"], rec["pre_players"], rec["mcts_records"][0], visits,
                                          rec["model_of"], rec["actions"], rec["material_balance"], rec["rewards"],
                                          rec["terminated"], rec["truncated"])
    s = stats.mcts
    assert (s.searched, s.noised, s.sampled, s.diverged) == (searched, searched, sampled, diverged)
    assert searched > 100 and 0 < diverged < sampled < searched
    # the samples: the visit words are the root visits, the recorded action is the move actually played
    ds, drained = arena.search_samples.drain()
    want = np.concatenate([rows[e, :meta[e, 1]] for e in range(N)])
    assert err == 0 and len(ds) == len(want) > 0 and drained.dropped == 0
    assert np.array_equal(ds.packed.cpu().numpy().view(np.uint32), want[:, :204])
    assert np.array_equal(ds.visits.cpu().numpy().view(np.uint32), want[:, 204:212])
