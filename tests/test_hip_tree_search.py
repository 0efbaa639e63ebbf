"""The tree search on the device: ka_search_advance against the float64 restatement on synthetic trees, its leaf q against
ka_lookahead_choose bit for bit, the forked nodes of every depth against replayed games bit for bit, the blunder of game (c),
the inactive cases, the error bits, and MatchArena(search=) ply by ply and move for move."""
import gc

import numpy as np
import pytest
import torch

from keisei_amd import _lib
from keisei_amd.shogi_gym import ACTION_SPACE, VecEnv
from keisei_amd.training import (LookaheadControls, MatchArena, SearchControls, TreeSearch, lookahead_active,
                                 lookahead_candidates, lookahead_choose, search_backup_select, search_expansions,
                                 search_leaf_q, search_records, search_table)
from keisei_amd.training.lookahead import (FLAG_ACTIVE, FLAG_CHANGED, FLAG_WON, REC_ACTION, REC_CAND, REC_FLAGS, REC_NCAND,
                                           REC_SLOT)
from keisei_amd.training.tree_search import FLAG_DEEPENED
from oracle import shogi as S
from policy_insight_helpers import ATOL, RTOL
from test_hip_lookahead_replies import (KING_HOME, MATE, MAX_PLY, N, PAIRINGS, PER, STEPS, _craft, _games, _group, _key,
                                        _lowest_legal, _scenario, _stream, _triples, _unpack)

pytestmark = pytest.mark.gpu
DEV = "cuda"
U24 = 2.0 ** -24                                              # the unit roundoff of fp32


@pytest.fixture(autouse=True)
def _release_device_objects():
    """Arenas own captured graphs and pinned buffers: collect them with the device idle, not inside a later test's capture."""
    yield
    gc.collect()
    torch.cuda.synchronize()
    gc.collect()


def _table(*controls):
    return torch.from_numpy(search_table(list(controls), len(controls))).to(DEV)


def _row(n_envs, W, e, node):
    return (node // W * n_envs + e) * W + node % W


# ------------------------------------------------------------------ 1. / 2. ka_search_advance alone
QS = (-0.6, -0.45, -0.2, 0.05, 0.1, 0.25, 0.35, 0.5, 0.7)      # every |q| differs from every other by at least 0.05


def _advance_alone(W, E, B, seed, weight, normal_logits=False):
    """Synthetic trees through ka_search_advance: every expansion's rows are made up for the parents the kernel chose.
    Yields after every launch ``(t, records, tree, parent_row, active, world)`` from the device."""
    rng = np.random.default_rng(seed)
    P = E * B * W
    if normal_logits:
        vl = rng.normal(0, 2.0, (E, B, W, 3)).astype(np.float32)
    else:
        vl = _triples(QS)[rng.integers(0, len(QS), (E, B, W))]
    done = rng.random((E, B, W)) < 0.15
    rewards = (rng.integers(-1, 2, (E, B, W)) * done).astype(np.float32)
    priors = (rng.integers(0, 3, (E, B, W)) / 2).astype(np.float32)
    n_all = rng.integers(0, W + 1, (E, B))
    n_all[1:][rng.random((E - 1, B)) < 0.8] = W               # most forks find every candidate
    n_all[0] = np.maximum(n_all[0], 1)
    n_all[0, :4] = [0, 1, W, W]
    cands = rng.integers(0, ACTION_SPACE, (E, B, W))
    ctl = [SearchControls(W, E, weight), SearchControls(W, min(E, 2), 0.0)]
    model_of = torch.from_numpy(rng.integers(0, 2, B).astype(np.int32)).to(DEV)
    table = _table(*ctl)
    d = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dt)  # noqa: E731
    pool_vl, pool_rw = d(vl.reshape(P, 3), torch.float32), d(rewards.reshape(P), torch.float32)
    pool_term, pool_trunc = d(done.reshape(P), torch.bool), torch.zeros(P, dtype=torch.bool, device=DEV)
    words = _lib.query("ka_search_words", 0, W, E)
    rec = torch.zeros(E, B, words, dtype=torch.int32, device=DEV)
    tree = torch.zeros(B, _lib.query("ka_search_words", 1, W, E), dtype=torch.int32, device=DEV)
    step_err = torch.zeros(E, 2, dtype=torch.int64, device=DEV)
    sampled = d(np.where(rng.random(B) < 0.5, cands[0, :, 0], 0), torch.int64)
    actions = sampled.clone()
    parent_row = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    active = torch.zeros(B, dtype=torch.int32, device=DEV)
    pv = torch.full((B, E), -9, dtype=torch.int32, device=DEV)
    counters = torch.zeros(6, dtype=torch.int32, device=DEV)
    world = dict(vl=vl, done=done, rewards=rewards, priors=priors, cands=cands, ctl=ctl, model_of=model_of.cpu().numpy(),
                 sampled=sampled.cpu().numpy(), actions=actions, pv=pv, counters=counters, table=table)
    for t in range(E):
        on = np.ones(B, bool) if t == 0 else active.cpu().numpy().astype(bool)
        n_t = np.where(on, n_all[t], 0)
        rec[t] = search_records(n_t[None], priors[t][None], None, cands[t][None])[0].to(DEV)
        _lib.call("ka_search_advance", rec, tree, W, E, t, table, model_of, 2, pool_vl, pool_rw, pool_term, pool_trunc,
                  step_err, actions, parent_row, active, pv, counters, counters.data_ptr() + 20, B, _stream())
        torch.cuda.synchronize()
        tr = tree.cpu()
        yield (t, rec.cpu(), {"parent": tr[:, :E].numpy(), "val": tr[:, E:E + E * W].contiguous().view(torch.float32).numpy(),
                              "by": tr[:, E + E * W:].numpy()}, parent_row.cpu().numpy(), active.cpu().numpy(), world)


@pytest.mark.parametrize("W,E,weight", [(1, 1, 0.0), (3, 4, 0.0371), (8, 16, 0.0371)])
def test_advance_is_the_restatement_on_synthetic_trees(W, E, weight):
    B = 64
    ran = deep = finished = 0
    for t, rec, tree, parent_row, active, w in _advance_alone(W, E, B, 70 + W, weight):
        T = t + 1
        parent = tree["parent"][:, :T].T
        want = search_backup_select(rec[:T], w["done"][:T], parent, w["ctl"], w["model_of"])
        u = np.sort(want.u, axis=1)[:, ::-1]                  # no root is ambiguous: gaps of 0 or at least 1e-3
        with np.errstate(invalid="ignore"):
            gaps = (u[:, :-1] - u[:, 1:])[np.isfinite(u[:, 1:])] if W > 1 else np.zeros(0)
        assert ((gaps == 0) | (gaps >= 1e-3)).all()
        # the leaf to fork next, the values, who forked what, and every record's first-maximum child
        rows = np.array([_row(B, W, e, n) if n >= 0 else -1 for e, n in enumerate(want.next_node)])
        assert np.array_equal(parent_row, rows) and np.array_equal(active, (rows >= 0).astype(np.int32)), t
        assert np.array_equal(tree["val"][:, :T * W].astype(np.float64), want.val.reshape(B, -1)), t     # exact: max and negation
        assert np.array_equal(tree["by"][:, :T * W], want.by.reshape(B, -1)), t
        if T < E:
            assert np.array_equal(tree["parent"][:, T], want.next_node), t
        for x in range(T):
            has = want.slot[x] >= 0
            assert np.array_equal(rec[x, :, REC_SLOT].numpy()[has], want.slot[x][has]), (t, x)
            got_a = rec[x, :, REC_ACTION].numpy()[has]
            assert np.array_equal(got_a, rec[x].numpy()[has, REC_CAND + want.slot[x][has]]), (t, x)
        ran += int((parent[t] >= 0).sum()) if t else int((rec[0, :, REC_FLAGS] & 1).ne(0).sum())
        finished += int(want.finished.sum())
    # behind the last expansion: the choice, the flags, the line and the counters
    root = (rec[0, :, REC_FLAGS] & FLAG_ACTIVE).ne(0).numpy()
    assert root.sum() == B - 1 and not root[0]
    choice = np.where(root, rec[0, :, REC_SLOT].numpy(), -1)
    assert np.array_equal(choice, want.choice)
    acts = w["actions"].cpu().numpy()
    chosen = rec[0].numpy()[np.arange(B), REC_CAND + np.maximum(choice, 0)]
    assert np.array_equal(acts, np.where(root, chosen, w["sampled"]))
    changed = root & (chosen != w["sampled"])
    won = root & w["done"][0, np.arange(B), np.maximum(choice, 0)] & (w["rewards"][0, np.arange(B), np.maximum(choice, 0)] > 0)
    flags = root * (1 + 2 * changed + 4 * won + 8 * want.deepened)
    assert np.array_equal(rec[0, :, REC_FLAGS].numpy(), flags)
    assert np.array_equal(w["pv"].cpu().numpy(), want.pv)
    deep = int(want.deepened.sum())
    assert w["counters"].cpu().tolist() == [int(root.sum()), int(changed.sum()), int(won.sum()), deep, ran, 0]
    if E > 1:
        assert deep >= 1 and finished >= 1 and ran > B and int(changed.sum()) >= 5 and int((~changed & root).sum()) >= 1


def test_leaf_q_is_what_lookahead_choose_writes_bit_for_bit():
    W, E, B = 3, 4, 64
    seen = 0
    for t, rec, tree, parent_row, active, w in _advance_alone(W, E, B, 91, 0.25, normal_logits=True):
        n = rec[t, :, REC_NCAND] * (rec[t, :, REC_FLAGS] & 1)
        one = lookahead_choose(torch.from_numpy(w["priors"][t]).to(DEV), n.to(DEV), torch.from_numpy(w["vl"][t]).to(DEV),
                               torch.from_numpy(w["rewards"][t]).to(DEV), torch.from_numpy(w["done"][t]).to(DEV), 0.25)
        used = (torch.arange(W)[None, :] < n[:, None])
        got = rec[t, :, REC_CAND + 2 * W:REC_CAND + 3 * W]
        assert torch.equal(got[used], one.q.cpu().view(torch.int32)[used]), t
        assert torch.equal(got[~used], torch.zeros_like(got[~used]))
        seen += int(used.sum())
    assert seen > 2 * B * W


# ------------------------------------------------------------------ the stages one by one
def _search(ts, env, logits, model_of, table, pre_step=None, post_eval=None):
    """clear, then per expansion: fork / expand, (pre_step), step, forward, (post_eval), advance.  Returns the actions and
    the sampled actions (the lowest legal move of every env)."""
    cur = env.current()
    sampled = torch.tensor(_lowest_legal(cur.legal_mask_bits), dtype=torch.int64, device=DEV)
    actions = sampled.clone()
    ts.clear()
    for t in range(ts.expansions):
        if t == 0:
            ts.fork(logits, cur.legal_mask_bits, actions, model_of, table, _stream())
        else:
            ts.expand(t, table, _stream())
        if pre_step is not None:
            pre_step(t)
        ts.step_nodes(t, _stream())
        ts.evaluate(t)
        if post_eval is not None:
            post_eval(t)
        ts.advance(t, actions, model_of, table, _stream())
    torch.cuda.synchronize()
    return actions, sampled


def _set_q(ts, t, qs):
    """value logits whose P(L) - P(W) is qs[j] in slot j of every env's rows of slice t"""
    s = ts.rows(t)
    ts.value_logits[s] = torch.from_numpy(_triples(qs)).to(DEV).repeat(ts.env.num_envs, 1)


# ------------------------------------------------------------------ 3. fork fidelity at every depth
@pytest.mark.parametrize("max_ply", [24, 23, 16, 15])      # (history rows copied in 16-, 8-, 4- and 1-byte pieces)
def test_forked_nodes_are_the_replayed_games_bit_for_bit(max_ply):
    """The four scripted games after 14 plies, width 3, three expansions, the value logits overwritten so that the line goes
    through the third candidate of the root and the third reply behind it.  At 24 and 23 the repetition of (a) and the mate
    of (c) happen at depth 2 and end those searches, (b) and (d) go to depth 3; at 16 every depth-2 node is truncated; at 15
    every depth-1 node is, and nothing more is forked."""
    W, E = 3, 3
    env, hist, start, logits, third, reply = _scenario(max_ply)
    ts = TreeSearch(env, _group(), W, E)
    table = _table(SearchControls(W, E))
    model_of = torch.zeros(4, dtype=torch.int32, device=DEV)
    rng = np.random.default_rng(10)

    def post_eval(t):
        _set_q(ts, t, [(-0.3, -0.3, 0.3), (-0.6, -0.6, -0.5), (0.1, 0.2, 0.3)][t])
        if t == 0 and max_ply != 15:                          # the interesting reply third behind the interesting move
            masks = _unpack(ts.mask_bits[ts.rows(0)])
            for e in (0, 2):
                ts.logits.reshape(-1, ACTION_SPACE)[e * W + 2] = _craft(rng, masks[e * W + 2], third=reply[e]).to(DEV)

    env_rows = (env._state, env._keys, env._checks, env.current().legal_mask_bits)
    before_env = [x.clone() for x in env_rows]
    slices = {}

    def pre_step(t):                                          # the earlier slices are only read
        slices[t] = [x[:t * ts.M].clone() for x in (ts.state, ts.keys, ts.checks, ts.mask_bits, ts.logits, ts.value_logits,
                                                     ts.rewards, ts.terminated, ts.model_of, ts.actions)]

    _search(ts, env, logits, model_of, table, pre_step, post_eval)
    assert all(torch.equal(x, y) for x, y in zip(before_env, env_rows))
    now = [x[:2 * ts.M] for x in (ts.state, ts.keys, ts.checks, ts.mask_bits, ts.logits, ts.value_logits, ts.rewards,
                                  ts.terminated, ts.model_of, ts.actions)]
    assert all(torch.equal(x, y) for x, y in zip(slices[2], now))
    assert not bool(ts._step_err.any())                       # no step was refused, the fallback rows' neither
    ts.read()
    rec, tree, pv = ts.records().cpu(), {k: v.cpu() for k, v in ts.tree().items()}, ts.principal_variations().cpu()
    parent = tree["parent"].numpy()
    assert rec[0, :, REC_NCAND].tolist() == [W] * 4
    done = (ts.terminated | ts.truncated).cpu().numpy().reshape(E, 4, W)
    if max_ply == 15:                                         # every child is truncated: three values of 0, the first is taken
        assert done[0].all() and (parent == -1).all() and not rec[1:, :, REC_FLAGS].any() and rec[0, :, REC_SLOT].tolist() == [0] * 4
    elif max_ply == 16:
        assert parent.tolist() == [[-1, 2, -1]] * 4 and done[1].all() and not done[0].any() and not rec[2, :, REC_FLAGS].any()
        assert rec[0, :, REC_SLOT].tolist() == [2] * 4
    else:
        # (a) ends in the repetition, a draw that stays the best line; in (c) the mate makes the third move the worst, and the
        # last expansion goes to the first move instead; (b) and (d) go down the line
        assert parent.tolist() == [[-1, 2, -1], [-1, 2, 5], [-1, 2, 0], [-1, 2, 5]] and rec[0, :, REC_SLOT].tolist() == [2, 2, 0, 2]
        assert int(rec[1, 0, REC_CAND + 2]) == reply[0] and int(rec[1, 2, REC_CAND + 2]) == MATE
        reason = ts.reason.cpu().numpy().reshape(E, 4, W)
        assert reason[1, 0].tolist() == [S.R_PROGRESS, S.R_PROGRESS, S.R_REPETITION] and float(ts.rewards[ts.M + 2]) == 0.0
        assert reason[1, 2].tolist() == [S.R_PROGRESS, S.R_PROGRESS, S.R_CHECKMATE] and float(ts.rewards[ts.M + 2 * W + 2]) == 1.0
        assert tree["val"][2, 0].tolist()[2] == -1.0 and tree["val"][0, 0].tolist()[2] == 0.0
        assert pv[2].tolist() == [int(rec[0, 2, REC_CAND]), int(rec[2, 2, REC_CAND + 2]), -1] and third[2] == KING_HOME
        assert pv[0].tolist() == [third[0], reply[0], -1] and pv[1, 2] >= 0 and pv[3, 2] >= 0
    # inactive rows of the later slices: the fallback's lowest legal action, no model
    lowest = _lowest_legal(ts.mask_bits[ts.rows(0)])
    for t in range(1, E):
        for e in range(4):
            s = slice(t * ts.M + e * W, t * ts.M + (e + 1) * W)
            if parent[e, t] < 0:
                assert ts.model_of[s].cpu().tolist() == [-1] * W and ts.actions[s].cpu().tolist() == [lowest[e * W]] * W, (t, e)
                assert int(rec[t, e, REC_FLAGS]) == 0 and int(rec[t, e, REC_ACTION]) == lowest[e * W]
            else:
                assert ts.model_of[s].cpu().tolist() == [0] * W and int(rec[t, e, REC_NCAND]) == W, (t, e)
                # the candidates are the restatement's, of the parent's own logits over its own mask
                p = _row(4, W, e, int(parent[e, t]))
                want_c, _, _ = lookahead_candidates(ts.logits.reshape(-1, ACTION_SPACE)[p:p + 1].cpu(), ts.mask_bits[p:p + 1].cpu(), W)
                assert rec[t, e, REC_CAND:REC_CAND + W].tolist() == want_c[0].tolist() == ts.actions[s].cpu().tolist(), (t, e)

    # a second env replays the history and then the path of every node that was forked for a candidate
    def path(e, node):
        acts = []
        while node >= 0:
            t, j = divmod(node, W)
            acts.append(int(rec[t, e, REC_CAND + j]))
            node = int(parent[e, t]) if t else -1
        return acts[::-1]

    nodes = [(e, t * W + j) for t in range(E) for e in range(4) for j in range(W) if t == 0 or parent[e, t] >= 0]
    depths = sorted({len(path(e, n)) for e, n in nodes})
    assert depths == ([1] if max_ply == 15 else [1, 2] if max_ply == 16 else [1, 2, 3])
    for depth in depths:
        group = [(e, n) for e, n in nodes if len(path(e, n)) == depth]
        rep = VecEnv(len(group), max_ply, "katago", "spatial", output="torch", check_actions=True)
        rep.reset()
        for g, (e, n) in enumerate(group):
            if e == 2:
                rep.set_state(g, *start)
        for k in range(STEPS + depth):
            acts = [hist[e][k] if k < STEPS else path(e, n)[k - STEPS] for e, n in group]
            r = rep.step(torch.tensor(acts, dtype=torch.int64, device=DEV))
        rows = torch.tensor([_row(4, W, e, n) for e, n in group], device=DEV)
        for name, got, want in (("packed mask", ts.mask_bits, r.legal_mask_bits), ("reward", ts.rewards, r.rewards),
                                ("terminated", ts.terminated, r.terminated), ("truncated", ts.truncated, r.truncated),
                                ("termination reason", ts.reason, r.step_metadata.termination_reason),
                                ("current player", ts.players, r.current_players), ("state", ts.state, rep._state)):
            assert got.dtype == want.dtype and torch.equal(got[rows], want), (name, depth)
        plies = rep._state[:, 100:104].contiguous().view(torch.int32).reshape(-1).cpu().tolist()
        for g, n_ply in enumerate(plies):                     # the history behind the node: entries [0, ply)
            n_ply = min(n_ply, rep._keys.shape[1])
            assert torch.equal(ts.keys[rows[g], :n_ply], rep._keys[g, :n_ply]), (depth, g)
            assert torch.equal(ts.checks[rows[g], :n_ply], rep._checks[g, :n_ply]), (depth, g)
        if depth == depths[-1] and max_ply in (24, 23):       # the observations of the last slice are still in the scratch
            assert torch.equal(ts.obs[rows - 2 * ts.M], r.observations)
    # later plies are not refused: the env plays the chosen moves
    actions = torch.tensor([int(a) for a in rec[0, :, REC_ACTION]], dtype=torch.int64, device=DEV)
    env.step(actions)
    env.raise_if_refused()


# ------------------------------------------------------------------ 4. the blunder of game (c)
def test_the_blunder_of_game_c_is_refused_at_two_expansions_and_played_at_one():
    W = 4
    env, hist, start, logits, _, _ = _scenario(24)
    ts = TreeSearch(env, _group(), W, 2)
    model_of = torch.zeros(4, dtype=torch.int32, device=DEV)
    masks = env.current().legal_masks.cpu().numpy()
    rng = np.random.default_rng(11)
    logits[2] = _craft(rng, masks[2], first=KING_HOME).to(DEV)
    c0 = 2 * W                                                # the node behind the king's move

    def post_eval(t):                                         # the mate is the third reply, and the value head likes the blunder
        if t == 0:
            ts.logits.reshape(-1, ACTION_SPACE)[c0] = _craft(rng, _unpack(ts.mask_bits[c0:c0 + 1])[0], third=MATE).to(DEV)
            ts.value_logits[c0] = torch.tensor([-4.0, 0.0, 4.0], device=DEV)

    actions, sampled = _search(ts, env, logits, model_of, _table(SearchControls(W, 2)), post_eval=post_eval)
    stats = ts.read()
    rec, tree, pv = ts.records().cpu(), ts.tree(), ts.principal_variations().cpu()
    assert int(rec[0, 2, REC_CAND]) == KING_HOME and int(tree["parent"][2, 1]) == 0 and int(tree["by"][2, 0, 0]) == 1
    assert rec[1, 2, REC_CAND:REC_CAND + 3].tolist()[2] == MATE and int(rec[1, 2, REC_SLOT]) == 2 and int(rec[1, 2, REC_ACTION]) == MATE
    assert rec.view(torch.float32)[1, 2, REC_CAND + 2 * W + 2].item() == 1.0     # the mate, for the player who gives it
    assert tree["val"][2, 0, 0].item() == -1.0                # val of the blunder, exactly
    assert rec.view(torch.float32)[0, 2, REC_CAND + 2 * W].item() > 0.9          # its leaf q stays in the record
    assert int(actions[2]) != KING_HOME and int(actions[2]) == int(rec[0, 2, REC_ACTION]) and int(rec[0, 2, REC_SLOT]) != 0
    assert int(rec[0, 2, REC_FLAGS]) & FLAG_DEEPENED and stats.deepened >= 1 and stats.searched == 4 and stats.expansions == 8
    assert stats.deepened == int((rec[0, :, REC_FLAGS] & FLAG_DEEPENED).ne(0).sum())
    assert pv[2].tolist() == [int(actions[2]), -1]            # the chosen move was never expanded
    r = env.step(actions)
    env.raise_if_refused()
    assert not bool(r.terminated[2])
    # with one expansion in the table the blunder is played, through the same two launches
    env, hist, start, logits2, _, _ = _scenario(24)
    logits2[2] = logits[2]
    ts = TreeSearch(env, _group(), W, 2)
    actions, sampled = _search(ts, env, logits2, model_of, _table(SearchControls(W, 1)), post_eval=post_eval)
    stats = ts.read()
    rec = ts.records().cpu()
    assert int(actions[2]) == KING_HOME and not int(rec[0, 2, REC_FLAGS]) & FLAG_DEEPENED and stats.deepened == 0
    assert stats.expansions == 4 and not rec[1, :, REC_FLAGS].any() and ts.principal_variations()[2].tolist() == [KING_HOME, -1]


# ------------------------------------------------------------------ 5. the inactive cases
def test_inactive_rows_get_the_fallback_action_and_no_model():
    W, E = 3, 4
    ctl = [SearchControls(W, E), SearchControls(W, 1), SearchControls(W, E, skip_plies=16), SearchControls.OFF]
    table = _table(*ctl)
    for model_of, live in (([0, 1, 2, -1], [0]), ([0, 0, 3, 0], [0, 1, 3])):
        env, hist, start, logits, third, reply = _scenario(24)
        ts = TreeSearch(env, _group(), W, E)
        mo = torch.tensor(model_of, dtype=torch.int32, device=DEV)
        rng = np.random.default_rng(12)

        def post_eval(t):                                     # env 0 ends in the repetition, a draw that stays its best line
            if t == 0:
                _set_q(ts, 0, (-0.3, -0.3, 0.3))
                c = 0 * W + 2
                ts.logits.reshape(-1, ACTION_SPACE)[c] = _craft(rng, _unpack(ts.mask_bits[c:c + 1])[0], third=reply[0]).to(DEV)
            else:
                _set_q(ts, t, (-0.6, -0.6, -0.5))

        actions, sampled = _search(ts, env, logits, mo, table, post_eval=post_eval)
        assert not bool(ts._step_err.any())                   # no step is refused
        stats = ts.read()
        rec, parent = ts.records().cpu(), ts.tree()["parent"].cpu().numpy()
        root = [m in (0, 1) for m in model_of]                # seated, on, past skip_plies
        assert [bool(f & FLAG_ACTIVE) for f in rec[0, :, REC_FLAGS].tolist()] == root
        assert [int(a) for a in actions] == [int(rec[0, e, REC_ACTION]) if root[e] else int(sampled[e]) for e in range(4)]
        lowest = _lowest_legal(ts.mask_bits[ts.rows(0)])
        for e in range(4):
            s0 = slice(e * W, (e + 1) * W)
            if not root[e]:                                   # expansion 0 of an inactive env: the sampler's action, no model
                assert ts.model_of[s0].cpu().tolist() == [-1] * W and ts.actions[s0].cpu().tolist() == [int(sampled[e])] * W
            for t in range(1, E):
                s = slice(t * ts.M + e * W, t * ts.M + (e + 1) * W)
                on = e in live and (t < 2 or e != 0)          # env 0 finishes behind expansion 1: its best line ends in a done node
                assert (parent[e, t] >= 0) == on, (model_of, e, t)
                if not on:
                    assert ts.model_of[s].cpu().tolist() == [-1] * W and ts.actions[s].cpu().tolist() == [lowest[e * W]] * W
                    assert int(rec[t, e, REC_FLAGS]) == 0 and int(rec[t, e, REC_NCAND]) == 0 and int(rec[t, e, REC_ACTION]) == lowest[e * W]
                else:
                    assert ts.model_of[s].cpu().tolist() == [model_of[e]] * W and int(rec[t, e, REC_FLAGS]) & FLAG_ACTIVE
        assert stats.searched == sum(root) and stats.expansions == sum(root) + int((parent >= 0).sum())
        env.step(actions)
        env.raise_if_refused()
    assert parent[0].tolist() == [-1, 2, -1, -1] and parent[1].tolist()[1] == 2 and (parent[[1, 3], 1:] >= 0).all()


# ------------------------------------------------------------------ 6. the error bits
def test_the_error_bits_raise_from_read():
    W, E = 3, 3
    env, hist, start, logits, _, _ = _scenario(24)
    ts = TreeSearch(env, _group(), W, E)
    table = _table(SearchControls(W, E))
    model_of = torch.zeros(4, dtype=torch.int32, device=DEV)
    _search(ts, env, logits, model_of, table)
    assert ts.read().searched == 4

    def nan_at_depth_2(t):
        if t == 1:
            row = ts.M + 1 * W                                # env 1 (pawn pushes): a live node of a live parent
            assert int(ts.model_of[row]) == 0 and not bool(ts.terminated[row] | ts.truncated[row])
            ts.value_logits[row, 2] = float("nan")
    _search(ts, env, logits, model_of, table, post_eval=nan_at_depth_2)
    with pytest.raises(RuntimeError, match="non-finite value logits in the search"):
        ts.read()
    assert np.isneginf(ts.records(1).cpu().view(torch.float32)[1, REC_CAND + 2 * W].item())
    assert np.isneginf(ts.tree()["val"][1, 1, 0].item())

    def mask_that_does_not_match(t):                          # the step validates every action against the row's mask
        if t == 1:
            ts.bits_in[ts.M + 1 * W].zero_()
    actions, sampled = _search(ts, env, logits, model_of, table, pre_step=mask_that_does_not_match)
    assert torch.equal(actions, sampled)                      # no action is replaced
    assert not bool(ts._step_err[0].any()) and bool(ts._step_err[1].any())
    with pytest.raises(RuntimeError, match="step of expansion 1 refused an action"):
        ts.read()
    ts.clear()
    assert ts.read() == type(ts.read())()
    actions, _ = _search(ts, env, logits, model_of, table)    # and the search works again
    assert ts.read().searched == 4
    env.step(actions)
    env.raise_if_refused()


# ------------------------------------------------------------------ 7. the recorded arena
CTL = [SearchControls(3, 4, 0.25), SearchControls(2, 1, 0.0, skip_plies=4)]
LA = [LookaheadControls(3, 0.25), LookaheadControls(2, 0.0, skip_plies=4)]


def test_every_recorded_arena_ply_is_the_restatement():
    grp = _group()
    arena = MatchArena(grp, N, PER, MAX_PLY, sync_every=2, graph=False, seed=21, record=True, search=CTL)
    assert arena.ply.stages["search"].engine.width == 3 and arena.ply.stages["search"].engine.expansions == 4
    results, stats = arena.run_round(PAIRINGS, games_per_match=4)
    recs = arena.record
    assert len(recs) >= 20 and stats.search.searched > 100
    table = search_table(CTL, 2)
    W, E = 3, 4
    bound = lambda w: 4 * U24 * (1 + w)                       # two fp32 roundings at magnitude <= 1 + w on each side  # noqa: E731
    selections = allowed = searched = changed = won = deepened = expansions = deep_lines = 0
    for ply, rec in enumerate(recs):
        mo = rec["model_of"]
        logits = grp.forward(rec["obs"].to(DEV), mo.to(DEV), check=False).policy_logits.reshape(N, ACTION_SPACE).cpu()
        widths, _ = lookahead_active(table, mo, rec["game_plies"], width=W)
        weights, exps = search_expansions(table, mo, expansions=E)
        cand, prior, n_cand = lookahead_candidates(logits, rec["mask_bits"], W)
        n_env = np.minimum(widths, n_cand.numpy())
        sr, tree, pv = rec["search_records"], rec["search_tree"], rec["search_pv"].numpy()
        parent = tree["parent"].numpy()
        q64, err = search_leaf_q(rec["node_value_logits"], rec["node_rewards"], rec["node_done"])
        node_c, node_p, node_n = lookahead_candidates(rec["node_logits"], rec["node_mask_bits"], W)
        wm = lookahead_active(table, mo, None, width=W)[0]    # the model's width: skip_plies plays no part below the root
        for e in range(N):
            n = int(n_env[e])
            flags = int(sr[0, e, REC_FLAGS])
            assert bool(flags & FLAG_ACTIVE) == (n > 0) and int(sr[0, e, REC_ACTION]) == int(rec["actions"][e]), (ply, e)
            if n == 0:
                assert flags == 0 and (parent[e] == -1).all() and (pv[e] == -1).all() and not sr[1:, e, REC_FLAGS].any(), (ply, e)
                continue
            assert int(sr[0, e, REC_NCAND]) == n and sr[0, e, REC_CAND:REC_CAND + W].tolist() == cand[e, :n].tolist() + [-1] * (W - n)
            for t in range(1, E):                             # the forks below the root: the parent's own logits and mask
                if parent[e, t] >= 0:
                    p = _row(N, W, e, int(parent[e, t]))
                    k = min(int(wm[e]), int(node_n[p]))
                    assert int(sr[t, e, REC_NCAND]) == k and sr[t, e, REC_CAND:REC_CAND + W].tolist() == node_c[p, :k].tolist() + [-1] * (W - k)
                    np.testing.assert_allclose(sr.view(torch.float32)[t, e, REC_CAND + W:REC_CAND + W + k].numpy().astype(np.float64),
                                               node_p[p, :k].numpy(), rtol=RTOL, atol=ATOL)
                    assert rec["node_model_of"][t, e, :k].tolist() == [int(mo[e])] * k
                else:
                    assert int(sr[t, e, REC_FLAGS]) == 0 and rec["node_model_of"][t, e].tolist() == [-1] * W
                kk = int(sr[t, e, REC_NCAND])
                np.testing.assert_allclose(sr.view(torch.float32)[t, e, REC_CAND + 2 * W:REC_CAND + 2 * W + kk].numpy().astype(np.float64),
                                           q64[t, e, :kk], rtol=RTOL, atol=ATOL)
        assert err == 0
        on = n_env > 0
        for T in range(1, E + 1):                             # every expansion, following the device's tree
            want = search_backup_select(sr[:T], rec["node_done"][:T], parent[:, :T].T, table, mo, q=q64[:T])
            for e in np.flatnonzero(on):
                selections += 1
                if T < E:
                    same = int(parent[e, T]) == int(want.next_node[e])
                else:
                    same = int(sr[0, e, REC_SLOT]) == int(want.choice[e]) and \
                        bool(int(sr[0, e, REC_FLAGS]) & FLAG_DEEPENED) == bool(want.deepened[e])
                    if same:
                        assert pv[e].tolist() == want.pv[e].tolist(), (ply, e)
                        for x in range(1, E):                 # below the root no difference is allowed
                            if want.slot[x, e] >= 0:
                                assert int(sr[x, e, REC_SLOT]) == int(want.slot[x, e]), (ply, e, x)
                if not same:                                  # only at the root of the model with a weight, inside the bound
                    u = np.sort(want.u[e][np.isfinite(want.u[e])])[::-1]
                    u1 = np.sort([q64[0, e, j] + weights[e] * float(prior[e, j]) for j in range(int(n_env[e]))])[::-1]
                    pick = int(sr[0, e, REC_SLOT]) if T == E else int(parent[e, T])       # the device's pick at the root
                    while pick >= W:
                        pick = int(parent[e, pick // W])
                    if pick >= 0 and pick != int(want.slot[0, e]):    # its float64 u lies within the bound of the maximum
                        close = u[0] - want.u[e][pick] <= bound(weights[e])
                    elif pick >= 0 and T == E:                # the same choice: the one-ply arg-max behind flag bit 3 is that close
                        close = len(u1) > 1 and u1[0] - u1[1] <= bound(weights[e])
                    elif pick < 0:                            # the device's line ended, its pick is not on record: the two best are that close
                        close = len(u) > 1 and u[0] - u[1] <= bound(weights[e])
                    else:                                     # the same pick at the root and a difference below it
                        close = False
                    assert weights[e] > 0 and close, (ply, e, T, u.tolist(), int(parent[e, min(T, E - 1)]), int(want.next_node[e]))
                    allowed += 1
        f = sr[0, :, REC_FLAGS].numpy()
        searched += int(on.sum())
        changed += int(((f & FLAG_CHANGED) != 0).sum())
        won += int(((f & FLAG_WON) != 0).sum())
        deepened += int(((f & FLAG_DEEPENED) != 0).sum())
        expansions += int(on.sum()) + int((parent >= 0).sum())
        deep_lines += int((pv[:, 2] >= 0).sum())
        assert ((exps[on] > 1) | (parent[on] == -1).all(1)).all()    # the expansions = 1 model forks nothing below the root
    print(f"active selections {selections}, inside the fp32 bound at the root with another pick {allowed}, searched {searched}, "
          f"changed {changed}, deepened {deepened}, expansions run {expansions}, lines of three moves or more {deep_lines}")
    s = stats.search
    assert (searched, changed, won, deepened, expansions) == (s.searched, s.changed, s.won, s.deepened, s.expansions)
    assert searched > 100 and expansions > 1.5 * searched
    assert allowed <= 0.02 * selections


def test_the_expansions_1_models_records_are_the_lookaheads_bit_for_bit():
    kw = dict(sync_every=2, graph=False, seed=22, record=True)
    search = MatchArena(_group(), N, PER, MAX_PLY, search=CTL, **kw)
    plain = MatchArena(_group(), N, PER, MAX_PLY, lookahead=LA, **kw)
    pairs = [(1, 1), (1, 1), (1, 1)]                          # the expansions = 1 model against itself, in four launches
    r0, s0 = search.run_round(pairs, games_per_match=4)
    r1, s1 = plain.run_round(pairs, games_per_match=4)
    assert _key(r0) == _key(r1) and len(search.record) == len(plain.record) >= 20
    for a, b in zip(search.record, plain.record):
        assert torch.equal(a["search_records"][0], b["lookahead_records"]) and torch.equal(a["actions"], b["actions"])
        assert not a["search_records"][1:, :, REC_FLAGS].any()
    s, la = s0.search, s1.lookahead
    assert (s.searched, s.changed, s.won, s.deepened, s.expansions) == (la.searched, la.changed, la.won, 0, la.searched) and s.searched > 50


# ------------------------------------------------------------------ 8. arena behaviour
def _arena(graph, seed=23, **kw):
    return MatchArena(_group(), N, PER, MAX_PLY, sync_every=2, graph=graph, seed=seed, game_log=256, **kw)


def test_graph_equals_no_graph():
    eager, graph = _arena(False, search=CTL), _arena(True, search=CTL)
    r1, s1 = eager.run_round(PAIRINGS, games_per_match=4)
    r2, s2 = graph.run_round(PAIRINGS, games_per_match=4)
    assert graph._graph is not None and eager._graph is None
    assert _key(r1) == _key(r2) and s1.round_plies == s2.round_plies and _games(r1) == _games(r2)
    assert s1.search == s2.search and s1.search.searched > 100 and s1.search.expansions > 1.5 * s1.search.searched
    assert torch.equal(eager.ply.stages["search"].engine.records(), graph.ply.stages["search"].engine.records()) and torch.equal(eager.ply.stages["search"].engine._tree, graph.ply.stages["search"].engine._tree)
    assert torch.equal(eager.ply.stages["search"].engine.principal_variations(), graph.ply.stages["search"].engine.principal_variations())
    assert torch.equal(eager.env.current().observations, graph.env.current().observations)


def test_rows_that_are_off_play_the_games_of_no_search_and_one_expansion_those_of_the_lookahead():
    none = _arena(True, seed=29)
    off = _arena(True, seed=29, search=[SearchControls.OFF, SearchControls(0, 1, 0.5)])
    assert "search" not in none.ply.stages and off.ply.stages["search"].engine is None and off.ply.stages["search"].table is not None     # nothing is allocated
    r0, s0 = none.run_round(PAIRINGS, games_per_match=4)
    r1, s1 = off.run_round(PAIRINGS, games_per_match=4)
    assert _key(r0) == _key(r1) and _games(r0) == _games(r1) and s0.search is None and s1.search == type(s1.search)()
    # an arena built for four expansions whose table is off: every launch runs, the same games move for move
    built = _arena(True, seed=29, search=CTL)
    built.set_search(None)
    r2, s2 = built.run_round(PAIRINGS, games_per_match=4)
    assert _key(r0) == _key(r2) and _games(r0) == _games(r2) and s2.search == type(s2.search)()
    # expansions = 1 everywhere: the games of the lookahead= arena
    plain = _arena(True, seed=29, lookahead=LA)
    built.set_search([SearchControls(3, 1, 0.25), SearchControls(2, 1, 0.0, skip_plies=4)])
    r3, s3 = plain.run_round(PAIRINGS, games_per_match=4)
    r4, s4 = built.run_round(PAIRINGS, games_per_match=4)
    assert _key(r3) == _key(r4) and _games(r3) == _games(r4) and _games(r3) != _games(r0)
    assert (s4.search.searched, s4.search.changed, s4.search.won) == (s3.lookahead.searched, s3.lookahead.changed, s3.lookahead.won)
    assert s4.search.deepened == 0 and s4.search.expansions == s4.search.searched > 100
    assert sum(len(g) for g in _games(r0)) >= 8


def test_set_search_rewrites_the_table_under_the_same_graph():
    arena, fresh = _arena(True, seed=31, search=CTL), _arena(True, seed=31, search=CTL)
    r0, s0 = arena.run_round(PAIRINGS, games_per_match=4)
    graph, table = arena._graph, arena.ply.stages["search"].table
    assert graph is not None and s0.search.expansions > 1.5 * s0.search.searched
    one = [SearchControls(3, 1, 0.25), SearchControls(2, 1, 0.0, skip_plies=4)]
    arena.set_search(one)
    assert table[:, 3].tolist() == [1, 1]
    r1, s1 = arena.run_round(PAIRINGS, games_per_match=4)
    assert s1.search.expansions == s1.search.searched > 100 and s1.search.deepened == 0
    arena.set_search(CTL)
    assert arena._graph is graph and arena.ply.stages["search"].table is table and table[:, 3].tolist() == [4, 1]
    r2, s2 = arena.run_round(PAIRINGS, games_per_match=4)
    f0, _ = fresh.run_round(PAIRINGS, games_per_match=4)      # the rounds depend on the table alone
    fresh.set_search(one)
    f1, _ = fresh.run_round(PAIRINGS, games_per_match=4)
    fresh.set_search(CTL)
    f2, t2 = fresh.run_round(PAIRINGS, games_per_match=4)
    assert _games(f0) == _games(r0) and _games(f1) == _games(r1) and _games(f2) == _games(r2) and t2.search == s2.search
    assert _games(r1) != _games(r0)


def test_refusals():
    with pytest.raises(ValueError, match="cannot be combined with lookahead="):
        MatchArena(_group(), N, PER, MAX_PLY, graph=False, search=CTL, lookahead=LA)
    with pytest.raises(ValueError, match="cannot be combined with collect=True"):
        MatchArena(_group(), N, PER, MAX_PLY, graph=False, search=CTL, collect=True)
    arena = MatchArena(_group(), N, PER, MAX_PLY, graph=False, search=CTL)
    with pytest.raises(ValueError, match="above the width"):
        arena.set_search(SearchControls(4, 2))
    with pytest.raises(ValueError, match="above the expansions"):
        arena.set_search(SearchControls(3, 5))
    arena.set_search(SearchControls(3, 4))
    with pytest.raises(ValueError, match="built without search="):
        MatchArena(_group(), N, PER, MAX_PLY, graph=False).set_search(CTL)
    env = VecEnv(4, 24, "katago", "spatial", output="torch", check_actions=True)
    env.reset()
    with pytest.raises(ValueError, match="expansions must be an integer"):
        TreeSearch(env, _group(), 3, 17)
    with pytest.raises(ValueError, match="width must be an integer"):
        TreeSearch(env, _group(), 0, 2)
    ts = TreeSearch(env, _group(), 3, 2)
    with pytest.raises(ValueError, match="lies outside"):
        ts.records(2)
    t = _table(SearchControls(3, 2))
    with pytest.raises(_lib.KeiseiHipError, match="expansion must lie in"):
        _lib.call("ka_search_advance", ts._records, ts._tree, 3, 2, 2, t, ts.active, 1, ts.value_logits, ts.rewards,
                  ts.terminated, ts.truncated, ts._step_err, ts.actions, ts.parent_row, ts.active, ts._pv, ts._counters,
                  ts._counters, 4, _stream())
    with pytest.raises(_lib.KeiseiHipError, match="slice 1 of the pool"):
        s = ts.rows(0)
        _lib.call("ka_search_expand", ts.logits, 0, ts.mask_bits, ts.mask_bits.shape[1], ts.model_of, 1, t, ts.state, ts.keys,
                  ts.checks, ts.terminated, ts.truncated, 24, 3, 1, ts.parent_row, ts.active, ts._records[1], ts.state[s],
                  ts.keys[s], ts.checks[s], ts.bits_in[s], ts.actions[s], ts.model_of[s], 4, ACTION_SPACE, _stream())
