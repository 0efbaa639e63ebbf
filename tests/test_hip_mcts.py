"""The visit-count search on the device: ka_mcts_advance against the float64 restatement on the synthetic worlds of
tests/mcts_helpers.py, its leaf q against ka_lookahead_choose bit for bit, the forked nodes of every depth against replayed
games bit for bit, the blunder of game (c), the error bits, and MatchArena(mcts=) ply by ply and move for move."""
import gc

import numpy as np
import pytest
import torch

import mate_search_helpers as MH
import mcts_helpers as H
from keisei_amd import _lib
from keisei_amd.shogi_gym import ACTION_SPACE, VecEnv
from keisei_amd.training import (LookaheadControls, MatchArena, MateControls, MctsControls, MctsRestatement, MctsSearch,
                                 SearchControls, lookahead_active, lookahead_candidates, lookahead_choose, mcts_backup_select,
                                 mcts_simulations, mcts_table, search_leaf_q, visit_policy)
from keisei_amd.training.lookahead import (FLAG_ACTIVE, FLAG_CHANGED, FLAG_WON, REC_ACTION, REC_CAND, REC_FLAGS, REC_NCAND,
                                           REC_SLOT)
from keisei_amd.training.tree_search import FLAG_DEEPENED
from policy_insight_helpers import ATOL, RTOL
from test_hip_lookahead_replies import (KING_HOME, MATE, MAX_PLY, N, PAIRINGS, PER, _craft, _games, _group, _key,
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
    return torch.from_numpy(mcts_table(list(controls), len(controls))).to(DEV)


def _row(n_envs, W, e, node):
    return (node // W * n_envs + e) * W + node % W


def _split(tree, E, W):
    """the tree words of every env as ka_mcts_advance lays them out"""
    t = tree.cpu()
    part = lambda i: t[:, E + i * E * W:E + (i + 1) * E * W].contiguous()  # noqa: E731
    return {"parent": t[:, :E].numpy(), "N": part(0).numpy(), "S": part(1).view(torch.float32).numpy(),
            "P": part(2).view(torch.float32).numpy(), "by": part(3).numpy()}


# ------------------------------------------------------------------ 1. ka_mcts_advance alone
def _advance_alone(world, normal_logits=None):
    """A synthetic world through ka_mcts_advance: every simulation's rows are made up for the nodes the kernel selected.
    Yields after every launch ``(t, records, tree, parent_row, active, buffers)`` from the device."""
    W, E, B = world["W"], world["E"], world["B"]
    P = E * B * W
    vl = world["vl"] if normal_logits is None else normal_logits
    d = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(device=DEV, dtype=dt)  # noqa: E731
    pool_vl, pool_rw = d(vl.reshape(P, 3), torch.float32), d(world["rewards"].reshape(P), torch.float32)
    pool_term, pool_trunc = d(world["done"].reshape(P), torch.bool), torch.zeros(P, dtype=torch.bool, device=DEV)
    words = _lib.query("ka_mcts_words", 0, W, E)
    rec = torch.zeros(E, B, words, dtype=torch.int32, device=DEV)
    tree = torch.full((B, _lib.query("ka_mcts_words", 1, W, E)), -5, dtype=torch.int32, device=DEV)
    step_err = torch.zeros(E, 2, dtype=torch.int64, device=DEV)
    buf = dict(actions=d(world["sampled"], torch.int64), pv=torch.full((B, E), -9, dtype=torch.int32, device=DEV),
               root_visits=torch.full((B, W), -9, dtype=torch.int32, device=DEV),
               root_values=torch.full((B, W), -9.0, dtype=torch.float32, device=DEV),
               counters=torch.zeros(7, dtype=torch.int32, device=DEV), table=_table(*world["ctl"]), step_err=step_err)
    model_of = d(world["model_of"], torch.int32)
    parent_row = torch.full((B,), -7, dtype=torch.int32, device=DEV)
    active = torch.zeros(B, dtype=torch.int32, device=DEV)
    out = []

    def advance(t, rec_t):
        rec[t] = torch.from_numpy(rec_t).to(DEV)
        _lib.call("ka_mcts_advance", rec, tree, W, E, t, buf["table"], model_of, 2, pool_vl, pool_rw, pool_term, pool_trunc,
                  step_err, buf["actions"], parent_row, active, buf["pv"], buf["root_visits"], buf["root_values"],
                  buf["counters"], buf["counters"].data_ptr() + 24, B, _stream())
        torch.cuda.synchronize()
        out.append((t, rec.cpu(), _split(tree, E, W), parent_row.cpu().numpy(), active.cpu().numpy(), buf))
        return out[-1][4]

    on = np.ones(B, bool)
    for t in range(E):
        on = np.asarray(advance(t, H.record_of(world, t, on)), bool)
        yield out[-1]


@pytest.mark.parametrize("W,E", H.SHAPES)
def test_advance_is_the_restatement_on_synthetic_worlds(W, E):
    """After every launch N, by, parent, the selected slots and parent_row / active are the restatement's exactly, and S lies
    within m^2 2^-24 of the float64 sum, m the node's visits: |q| <= 1, so a partial sum is at most m and each of the m fp32
    adds rounds by at most 2^-24 m.  The gap condition of tests/test_mcts_cpu.py is asserted again along the kernel's own
    path, with the kernel's own S: no selection is left out."""
    B = H.B
    world = H.make_world(W, E, H.SEEDS[W, E])
    r = MctsRestatement(world["ctl"], world["model_of"], B, W, E)
    ran = revisits = levels = 0
    for t, rec, tree, parent_row, active, buf in _advance_alone(world):
        T = t + 1
        r.advance(rec[t], world["done"][t], tree["parent"][:, t])      # the kernel's own records (its fp32 q) and its path
        want = r.tree()
        # every selection made behind this launch: no two best scores closer than fp32 can tell, by the kernel's own operands
        for b, sel in enumerate(want.selections[t]):
            assert H.gap_violations(sel, tree["N"][b], tree["S"][b], tree["P"][b], W, r.S[b].reshape(-1)) == [], (t, b)
            levels += len(sel)
        rows = np.array([_row(B, W, e, n) if f else -1 for e, (n, f) in enumerate(zip(want.next_node, want.fork_next))])
        assert np.array_equal(parent_row, rows) and np.array_equal(active, want.fork_next.astype(np.int32)), t
        if T < E:
            assert np.array_equal(tree["parent"][:, T], want.next_node), t
        assert np.array_equal(tree["parent"][:, :T], r.parent[:T].T), t
        assert np.array_equal(tree["N"][:, :T * W], want.N.reshape(B, -1)), t
        assert np.array_equal(tree["by"][:, :T * W], want.by.reshape(B, -1)), t
        assert np.array_equal(tree["P"][:, :T * W].astype(np.float64), want.P.reshape(B, -1)), t
        m = want.N.reshape(B, -1).astype(np.float64)
        assert (np.abs(tree["S"][:, :T * W].astype(np.float64) - want.S.reshape(B, -1)) <= m * m * U24).all(), t
        assert np.array_equal(tree["S"][:, :T * W], want.S32.reshape(B, -1)), t      # and the fp32 sums in the kernel's order, exactly
        for x in range(1 if T == E else 0, T):                # the slot last selected among every simulation's children (the last
            #                                                   launch writes the choice into the root's record: below)
            has = want.slot[x] >= 0
            assert np.array_equal(rec[x, :, REC_SLOT].numpy()[has], want.slot[x][has]), (t, x)
            assert np.array_equal(rec[x, :, REC_ACTION].numpy()[has], rec[x].numpy()[has, REC_CAND + want.slot[x][has]]), (t, x)
        ran += int(want.ran[t].sum())
        revisits += int(want.revisit[t].sum())
        assert buf["counters"].cpu().tolist()[4:] == [ran, revisits, 0], t
    # behind the last launch: the choice, the flags, the line, the root's visits and the counters
    root = (rec[0, :, REC_FLAGS] & FLAG_ACTIVE).ne(0).numpy()
    assert root.sum() == B - 1 and not root[0] and int(rec[0, 1, REC_NCAND]) == 1
    choice = np.where(root, rec[0, :, REC_SLOT].numpy(), -1)
    assert np.array_equal(choice, want.choice)
    acts = buf["actions"].cpu().numpy()
    chosen = rec[0].numpy()[np.arange(B), REC_CAND + np.maximum(choice, 0)]
    assert np.array_equal(acts, np.where(root, chosen, world["sampled"]))      # untouched rows keep the sampler's action
    changed = root & (chosen != world["sampled"])
    at = (0, np.arange(B), np.maximum(choice, 0))
    won = root & world["done"][at] & (world["rewards"][at] > 0)
    flags = root * (1 + 2 * changed + 4 * won + 8 * want.deepened)
    assert np.array_equal(rec[0, :, REC_FLAGS].numpy(), flags)
    assert np.array_equal(buf["pv"].cpu().numpy(), want.pv)
    assert np.array_equal(buf["root_visits"].cpu().numpy(), want.visits)
    assert np.abs(buf["root_values"].cpu().numpy().astype(np.float64) - want.mean).max() <= 64 * U24 + 2 * U24
    deep = int(want.deepened.sum())
    assert buf["counters"].cpu().tolist() == [int(root.sum()), int(changed.sum()), int(won.sum()), deep, ran, revisits, 0]
    # the restatement in one call says the same
    once = mcts_backup_select(rec, world["done"], tree["parent"].T, world["ctl"], world["model_of"])
    for name in ("N", "S", "by", "choice", "pv", "deepened", "revisit"):
        assert np.array_equal(getattr(once, name), getattr(want, name)), name
    sims = mcts_simulations(world["ctl"], world["model_of"], simulations=E)[1]
    assert np.array_equal(want.ran.sum(0), np.where(root, sims, 0))            # every model ran its own simulations
    if E > 1:
        assert deep >= 1 and revisits >= 1 and ran > B and int(changed.sum()) >= 1 and int((~changed & root).sum()) >= 1
        assert levels > B * (E - 1) // 2 and len(set(sims[root].tolist())) == 2


# ------------------------------------------------------------------ 3. the leaf q
def test_leaf_q_is_what_lookahead_choose_writes_bit_for_bit():
    W, E, B = 3, 4, 64
    world = H.make_world(W, E, 91)
    vl = np.random.default_rng(91).normal(0, 2.0, (E, B, W, 3)).astype(np.float32)
    seen = 0
    for t, rec, tree, parent_row, active, buf in _advance_alone(world, normal_logits=vl):
        n = rec[t, :, REC_NCAND] * (rec[t, :, REC_FLAGS] & 1)
        one = lookahead_choose(torch.from_numpy(world["priors"][t]).to(DEV), n.to(DEV), torch.from_numpy(vl[t]).to(DEV),
                               torch.from_numpy(world["rewards"][t]).to(DEV), torch.from_numpy(world["done"][t]).to(DEV), 0.25)
        used = (torch.arange(W)[None, :] < n[:, None])
        got = rec[t, :, REC_CAND + 2 * W:REC_CAND + 3 * W]
        assert torch.equal(got[used], one.q.cpu().view(torch.int32)[used]), t
        assert torch.equal(got[~used], torch.zeros_like(got[~used]))
        if t == 0:                                            # slice 0: every active root, and the sums start from these bits
            assert int(used.sum()) >= B and np.array_equal(tree["S"][:, :W].view(np.int32)[used.numpy()], got[used].numpy())
        seen += int(used.sum())
    assert seen > 3 * B * W // 2                              # the roots' children and as many again below them


# ------------------------------------------------------------------ the stages one by one
def _search(ms, env, logits, model_of, table, pre_step=None, post_eval=None):
    """clear, then per simulation: fork / expand, (pre_step), step, forward, (post_eval), advance.  Returns the actions and
    the sampled actions (the lowest legal move of every env)."""
    cur = env.current()
    sampled = torch.tensor(_lowest_legal(cur.legal_mask_bits), dtype=torch.int64, device=DEV)
    actions = sampled.clone()
    ms.clear()
    for t in range(ms.simulations):
        if t == 0:
            ms.fork(logits, cur.legal_mask_bits, actions, model_of, table, _stream())
        else:
            ms.expand(t, table, _stream())
        if pre_step is not None:
            pre_step(t)
        ms.step_nodes(t, _stream())
        ms.evaluate(t)
        if post_eval is not None:
            post_eval(t)
        ms.advance(t, actions, model_of, table, _stream())
    torch.cuda.synchronize()
    return actions, sampled


def _set_q(ms, t, qs):
    """value logits whose P(L) - P(W) is qs[j] in slot j of every env's rows of slice t"""
    s = ms.rows(t)
    ms.value_logits[s] = torch.from_numpy(_triples(qs)).to(DEV).repeat(ms.env.num_envs, 1)


# ------------------------------------------------------------------ 2. fork fidelity at every depth
def test_forked_nodes_are_the_replayed_games_bit_for_bit():
    """8 envs after 6 plies of their own, width 3, 6 simulations by the models' own logits and values: every forked node's
    state, history, masks and step outputs are those of a second env that replays the game and then the node's path."""
    W, E, n, plies, max_ply = 3, 6, 8, 6, 24
    rng = np.random.default_rng(14)
    env = VecEnv(n, max_ply, "katago", "spatial", output="torch", check_actions=True)
    env.reset()
    hist = [[] for _ in range(n)]
    for k in range(plies):
        masks = _unpack(env.current().legal_mask_bits)
        acts = [int(rng.choice(np.flatnonzero(masks[e]))) for e in range(n)]
        for e in range(n):
            hist[e].append(acts[e])
        env.step(torch.tensor(acts, dtype=torch.int64, device=DEV))
    grp = _group()
    model_of = torch.tensor([0, 1] * (n // 2), dtype=torch.int32, device=DEV)
    logits = grp.forward(env.current().observations, model_of, check=False).policy_logits.reshape(n, ACTION_SPACE).clone()
    ms = MctsSearch(env, grp, W, E)
    table = _table(MctsControls(W, E, 1.25), MctsControls(W, E, 0.3))
    env_rows = (env._state, env._keys, env._checks, env.current().legal_mask_bits)
    before_env = [x.clone() for x in env_rows]
    slices = {}

    def pre_step(t):                                          # the earlier slices are only read
        slices[t] = [x[:t * ms.M].clone() for x in (ms.state, ms.keys, ms.checks, ms.mask_bits, ms.logits, ms.value_logits,
                                                     ms.rewards, ms.terminated, ms.model_of, ms.actions)]

    actions, _ = _search(ms, env, logits, model_of, table, pre_step)
    assert all(torch.equal(x, y) for x, y in zip(before_env, env_rows))
    now = [x[:(E - 1) * ms.M] for x in (ms.state, ms.keys, ms.checks, ms.mask_bits, ms.logits, ms.value_logits, ms.rewards,
                                        ms.terminated, ms.model_of, ms.actions)]
    assert all(torch.equal(x, y) for x, y in zip(slices[E - 1], now))
    assert not bool(ms._step_err.any())                       # no step was refused, the fallback rows' neither
    stats = ms.read()
    rec, tree = ms.records().cpu(), {k: v.cpu().numpy() for k, v in ms.tree().items()}
    parent, by = tree["parent"], tree["by"].reshape(n, -1)
    assert stats.searched == n and stats.simulations == n * E and rec[0, :, REC_NCAND].tolist() == [W] * n
    forked = np.array([[t == 0 or (parent[e, t] >= 0 and by[e, parent[e, t]] == t) for t in range(E)] for e in range(n)])
    assert stats.revisits == int((~forked).sum()) and forked.sum() > n * E // 2
    for e in range(n):                                        # the candidates are the restatement's, of the parent's own logits
        for t in range(1, E):
            s = slice(t * ms.M + e * W, t * ms.M + (e + 1) * W)
            if not forked[e, t]:
                assert int(rec[t, e, REC_FLAGS]) == 0 and ms.model_of[s].cpu().tolist() == [-1] * W
                continue
            p = _row(n, W, e, int(parent[e, t]))
            want_c, _, want_n = lookahead_candidates(ms.logits.reshape(-1, ACTION_SPACE)[p:p + 1].cpu(), ms.mask_bits[p:p + 1].cpu(), W)
            k = int(want_n[0])
            assert rec[t, e, REC_CAND:REC_CAND + k].tolist() == want_c[0, :k].tolist() == ms.actions[s].cpu().tolist()[:k], (t, e)
            assert ms.model_of[s].cpu().tolist()[:k] == [int(model_of[e])] * k

    def path(e, node):
        acts = []
        while node >= 0:
            t, j = divmod(node, W)
            acts.append(int(rec[t, e, REC_CAND + j]))
            node = int(parent[e, t]) if t else -1
        return acts[::-1]

    nodes = [(e, t * W + j) for e in range(n) for t in range(E) if forked[e, t] for j in range(int(rec[t, e, REC_NCAND]))]
    depths = sorted({len(path(e, nd)) for e, nd in nodes})
    assert depths[0] == 1 and len(depths) >= 3                # three plies deep at the least
    for depth in depths:
        group = [(e, nd) for e, nd in nodes if len(path(e, nd)) == depth]
        rep = VecEnv(len(group), max_ply, "katago", "spatial", output="torch", check_actions=True)
        rep.reset()
        for k in range(plies + depth):
            acts = [hist[e][k] if k < plies else path(e, nd)[k - plies] for e, nd in group]
            r = rep.step(torch.tensor(acts, dtype=torch.int64, device=DEV))
        rows = torch.tensor([_row(n, W, e, nd) for e, nd in group], device=DEV)
        for name, got, want in (("packed mask", ms.mask_bits, r.legal_mask_bits), ("reward", ms.rewards, r.rewards),
                                ("terminated", ms.terminated, r.terminated), ("truncated", ms.truncated, r.truncated),
                                ("termination reason", ms.reason, r.step_metadata.termination_reason),
                                ("current player", ms.players, r.current_players), ("state", ms.state, rep._state)):
            assert got.dtype == want.dtype and torch.equal(got[rows], want), (name, depth)
        counts = rep._state[:, 100:104].contiguous().view(torch.int32).reshape(-1).cpu().tolist()
        for g, n_ply in enumerate(counts):                    # the history behind the node: entries [0, ply)
            n_ply = min(n_ply, rep._keys.shape[1])
            assert torch.equal(ms.keys[rows[g], :n_ply], rep._keys[g, :n_ply]), (depth, g)
            assert torch.equal(ms.checks[rows[g], :n_ply], rep._checks[g, :n_ply]), (depth, g)
    # the visit distribution of the searched positions, and the env plays the chosen moves
    cand, visits, mean = ms.root_visits()
    assert torch.equal(cand.cpu(), rec[0, :, REC_CAND:REC_CAND + W]) and visits.sum(1).tolist() == [W + E - 1] * n
    assert torch.equal(visits.cpu(), torch.from_numpy(tree["N"][:, 0])) and bool((mean.abs() <= 1).all())
    target = visit_policy(cand, visits)
    assert target.shape == (n, ACTION_SPACE) and torch.allclose(target.sum(1), torch.ones(n, device=DEV), atol=1e-6)
    assert bool((target.gather(1, cand.long()) > 0).all()) and int((target > 0).sum()) == n * W
    assert torch.equal(visit_policy(cand, visits, 0).argmax(1), actions)
    env.step(actions)
    env.raise_if_refused()


# ------------------------------------------------------------------ 4. the blunder of game (c)
def test_the_blunder_of_game_c_is_left_with_enough_simulations_and_played_with_one():
    """Game (c): the top-logit move, the king's step home, walks into a mate in one, and the value head likes it (0.96).
    Greedy on the mean (c_puct 0), the other candidates at 0.3, -0.3, -0.3 and every deeper node at -0.2: simulation 1 goes
    down the blunder, finds the mate behind it (v = 1) and leaves it at a mean of -0.02; every later simulation goes down the
    second candidate, whose mean stays above 0.  Eight simulations: 2 visits against 7."""
    W, E = 4, 8
    env, hist, start, logits, _, _ = _scenario(24)
    ms = MctsSearch(env, _group(), W, E)
    model_of = torch.zeros(4, dtype=torch.int32, device=DEV)
    masks = env.current().legal_masks.cpu().numpy()
    rng = np.random.default_rng(11)
    logits[2] = _craft(rng, masks[2], first=KING_HOME).to(DEV)
    c0 = 2 * W                                                # the node behind the king's move

    def post_eval(t):                                         # the mate is the third reply, and the value head likes the blunder
        if t == 0:
            _set_q(ms, 0, (0.3, 0.3, -0.3, -0.3))
            ms.logits.reshape(-1, ACTION_SPACE)[c0] = _craft(rng, _unpack(ms.mask_bits[c0:c0 + 1])[0], third=MATE).to(DEV)
            ms.value_logits[c0] = torch.tensor([-4.0, 0.0, 4.0], device=DEV)
        else:
            _set_q(ms, t, (-0.2, -0.2, -0.2, -0.2))

    actions, sampled = _search(ms, env, logits, model_of, _table(MctsControls(W, E, 0.0)), post_eval=post_eval)
    stats = ms.read()
    rec, tree, pv = ms.records().cpu(), {k: v.cpu() for k, v in ms.tree().items()}, ms.principal_variations().cpu()
    assert int(rec[0, 2, REC_CAND]) == KING_HOME and int(tree["parent"][2, 1]) == 0 and int(tree["by"][2, 0, 0]) == 1
    assert rec[1, 2, REC_CAND:REC_CAND + 3].tolist()[2] == MATE
    assert rec.view(torch.float32)[1, 2, REC_CAND + 2 * W + 2].item() == 1.0     # the mate, for the player who gives it
    q0 = rec.view(torch.float32)[0, 2, REC_CAND + 2 * W].item()
    assert q0 > 0.9                                           # the blunder's leaf q stays in the record
    assert tree["N"][2, 0].tolist() == [2, 7, 1, 1] and tree["S"][2, 0, 0].item() == np.float32(q0) - np.float32(1.0)
    assert tree["parent"][2].tolist()[2] == 1 and (tree["parent"][2, 2:] > 0).all()
    assert int(actions[2]) == int(rec[0, 2, REC_CAND + 1]) == int(rec[0, 2, REC_ACTION]) and int(rec[0, 2, REC_SLOT]) == 1
    assert int(rec[0, 2, REC_FLAGS]) & FLAG_DEEPENED and stats.deepened >= 1 and stats.searched == 4
    assert stats.deepened == int((rec[0, :, REC_FLAGS] & FLAG_DEEPENED).ne(0).sum()) and stats.simulations == 4 * E
    assert pv[2, 0] == actions[2] and (pv[2, :3] >= 0).all() and pv[2, E - 1] == -1       # the line runs down the second candidate
    cand, visits, mean = ms.root_visits()
    assert visits[2].tolist() == [2, 7, 1, 1] and mean[2, 0].item() < 0 < mean[2, 1].item()
    r = env.step(actions)
    env.raise_if_refused()
    assert not bool(r.terminated[2])
    # with one simulation in the table the blunder is played, through the same launches
    env, hist, start, logits2, _, _ = _scenario(24)
    logits2[2] = logits[2]
    ms = MctsSearch(env, _group(), W, E)
    actions, sampled = _search(ms, env, logits2, model_of, _table(MctsControls(W, 1, 0.0)), post_eval=post_eval)
    stats = ms.read()
    rec = ms.records().cpu()
    assert int(actions[2]) == KING_HOME and not int(rec[0, 2, REC_FLAGS]) & FLAG_DEEPENED and stats.deepened == 0
    assert stats.simulations == 4 and stats.revisits == 0 and not rec[1:, :, REC_FLAGS].any()
    assert ms.principal_variations()[2].tolist() == [KING_HOME] + [-1] * (E - 1) and ms.root_visits()[1][2].tolist() == [1] * W


# ------------------------------------------------------------------ 5. the error bits
def test_the_error_bits_raise_from_read():
    W, E = 3, 4
    env, hist, start, logits, _, _ = _scenario(24)
    ms = MctsSearch(env, _group(), W, E)
    table = _table(MctsControls(W, E, 0.5))
    model_of = torch.zeros(4, dtype=torch.int32, device=DEV)
    _search(ms, env, logits, model_of, table)
    assert ms.read().searched == 4

    hit = []

    def nan_below_the_root(t):
        if t == 1:
            row = ms.M + 1 * W                                # env 1 (pawn pushes): a live node of a live parent
            assert int(ms.model_of[row]) == 0 and not bool(ms.terminated[row] | ms.truncated[row])
            ms.value_logits[row, 2] = float("nan")
            hit.append(row)
    _search(ms, env, logits, model_of, table, post_eval=nan_below_the_root)
    with pytest.raises(RuntimeError, match="non-finite value logits in the visit-count search"):
        ms.read()
    assert hit and ms.records(1).cpu().view(torch.float32)[1, REC_CAND + 2 * W].item() == 0.0    # its q reads as 0
    tree = ms.tree()
    assert bool(torch.isfinite(tree["S"]).all()) and bool(torch.isfinite(tree["P"]).all())       # no NaN in any tree
    assert bool(torch.isfinite(ms.root_visits()[2]).all()) and tree["N"][:, 0].sum(1).tolist() == [W + E - 1] * 4

    def mask_that_does_not_match(t):                          # the step validates every action against the row's mask
        if t == 1:
            ms.bits_in[ms.M + 1 * W].zero_()
    state_before = None

    def pre_step(t):
        nonlocal state_before
        mask_that_does_not_match(t)
        if t == 1:
            state_before = ms.state[ms.rows(1)].clone()
    actions, sampled = _search(ms, env, logits, model_of, table, pre_step=pre_step)
    assert torch.equal(actions, sampled)                      # no action is replaced
    assert not bool(ms._step_err[0].any()) and bool(ms._step_err[1].any())
    assert torch.equal(ms.state[ms.rows(1)], state_before)    # and the refused step moved no row of its slice
    with pytest.raises(RuntimeError, match="step of simulation 1 refused an action"):
        ms.read()
    ms.clear()
    assert ms.read() == type(ms.read())()
    actions, _ = _search(ms, env, logits, model_of, table)    # and the search works again
    assert ms.read().searched == 4
    env.step(actions)
    env.raise_if_refused()


# ------------------------------------------------------------------ 6. the arena
CTL = [MctsControls(3, 6, 1.25), MctsControls(2, 2, 0.0, skip_plies=4)]
ONE = [MctsControls(3, 1, 1.25), MctsControls(2, 1, 0.0, skip_plies=4)]


def test_every_recorded_arena_ply_is_the_restatement():
    """The eager stage sequence, ply by ply, following the device's tree: the candidates of every fork are the parent's own,
    the leaf q are search_leaf_q's, N / by are the restatement's exactly and S within m^2 2^-24.  The values are a network's,
    so a selection may have two scores closer than fp32 can tell: where the device went another way than the restatement
    the two best float64 scores of a level it passed lie within 1e-5 -- a mean is S / N with S off by at most m^2 2^-24 <= 36 *
    6e-8, and the prior term a few roundings at a magnitude below 1.25 * sqrt(8) -- and such selections are few."""
    grp = _group()
    arena = MatchArena(grp, N, PER, MAX_PLY, sync_every=2, graph=False, seed=21, record=True, mcts=CTL)
    assert arena.mcts.width == 3 and arena.mcts.simulations == 6
    results, stats = arena.run_round(PAIRINGS, games_per_match=4)
    recs = arena.record
    assert len(recs) >= 20 and stats.mcts.searched > 100
    table = mcts_table(CTL, 2)
    W, E = 3, 6
    selections = other = searched = changed = won = deepened = sims = revisits = 0
    for ply, rec in enumerate(recs):
        mo = rec["model_of"]
        logits = grp.forward(rec["obs"].to(DEV), mo.to(DEV), check=False).policy_logits.reshape(N, ACTION_SPACE).cpu()
        widths, _ = lookahead_active(table, mo, rec["game_plies"], width=W)
        cand, prior, n_cand = lookahead_candidates(logits, rec["mask_bits"], W)
        n_env = np.minimum(widths, n_cand.numpy())
        sr, tree, pv = rec["mcts_records"], {k: v.numpy() for k, v in rec["mcts_tree"].items()}, rec["mcts_pv"].numpy()
        parent = tree["parent"]
        q64, err = search_leaf_q(rec["node_value_logits"], rec["node_rewards"], rec["node_done"])
        assert err == 0
        for e in range(N):
            n = int(n_env[e])
            flags = int(sr[0, e, REC_FLAGS])
            assert bool(flags & FLAG_ACTIVE) == (n > 0) and int(sr[0, e, REC_ACTION]) == int(rec["actions"][e]), (ply, e)
            if n == 0:
                assert flags == 0 and (parent[e] == -1).all() and (pv[e] == -1).all() and not sr[1:, e, REC_FLAGS].any(), (ply, e)
                continue
            assert int(sr[0, e, REC_NCAND]) == n and sr[0, e, REC_CAND:REC_CAND + W].tolist() == cand[e, :n].tolist() + [-1] * (W - n)
            for t in range(E):
                kk = int(sr[t, e, REC_NCAND]) * (int(sr[t, e, REC_FLAGS]) & 1)
                np.testing.assert_allclose(sr.view(torch.float32)[t, e, REC_CAND + 2 * W:REC_CAND + 2 * W + kk].numpy().astype(np.float64),
                                           q64[t, e, :kk], rtol=RTOL, atol=ATOL)
        r = MctsRestatement(table, mo, N, W, E)
        on = n_env > 0
        for t in range(E):                                    # every simulation, following the device's tree
            r.advance(sr[t], rec["node_done"][t], parent[:, t])
            want = r.tree()
            for e in np.flatnonzero(on):
                selections += 1
                went = int(parent[e, t + 1]) if t + 1 < E else -1
                if t + 1 < E and went != int(want.next_node[e]):
                    gaps = [np.sort(s)[-1] - np.sort(s)[-2] for _, s, _ in want.selections[t][e] if len(s) > 1]
                    assert gaps and min(gaps) <= 1e-5, (ply, e, t, went, int(want.next_node[e]), gaps)
                    other += 1
        T = E * W
        assert np.array_equal(tree["N"].reshape(N, T)[on], want.N.reshape(N, T)[on]), ply
        m = want.N.reshape(N, T).astype(np.float64)
        assert (np.abs(tree["S"].reshape(N, T).astype(np.float64) - want.S.reshape(N, T))[on] <= (m * m * U24)[on]).all(), ply
        assert np.array_equal(tree["S"].reshape(N, T)[on], want.S32.reshape(N, T)[on]), ply
        assert np.array_equal(sr[0, :, REC_SLOT].numpy()[on], want.choice[on]) and np.array_equal(pv[on], want.pv[on]), ply
        f = sr[0, :, REC_FLAGS].numpy()
        assert np.array_equal((f & FLAG_DEEPENED) != 0, want.deepened), ply
        cand_r, visits, mean = rec["mcts_root_visits"]
        assert np.array_equal(visits.numpy(), want.visits) and np.abs(mean.numpy() - want.mean).max() <= 1e-6
        searched += int(on.sum())
        changed += int(((f & FLAG_CHANGED) != 0).sum())
        won += int(((f & FLAG_WON) != 0).sum())
        deepened += int(((f & FLAG_DEEPENED) != 0).sum())
        sims += int(want.ran.sum())
        revisits += int(want.revisit.sum())
    print(f"active selections {selections}, another way inside the fp32 bound {other}, searched {searched}, changed {changed}, "
          f"deepened {deepened}, simulations run {sims}, revisits {revisits}")
    s = stats.mcts
    assert (searched, changed, won, deepened, sims, revisits) == (s.searched, s.changed, s.won, s.deepened, s.simulations, s.revisits)
    assert searched > 100 and sims > 2 * searched
    assert other <= 0.02 * selections


def _arena(graph, seed=23, **kw):
    return MatchArena(_group(), N, PER, MAX_PLY, sync_every=2, graph=graph, seed=seed, game_log=256, **kw)


def test_graph_equals_no_graph_move_for_move():
    eager, graph = _arena(False, mcts=CTL), _arena(True, mcts=CTL)
    r1, s1 = eager.run_round(PAIRINGS, games_per_match=4)
    r2, s2 = graph.run_round(PAIRINGS, games_per_match=4)
    assert graph._graph is not None and eager._graph is None
    assert _key(r1) == _key(r2) and s1.round_plies == s2.round_plies and _games(r1) == _games(r2)
    assert s1.mcts == s2.mcts and s1.mcts.searched > 100 and s1.mcts.simulations > 2 * s1.mcts.searched
    assert torch.equal(eager.mcts.records(), graph.mcts.records()) and torch.equal(eager.mcts._tree, graph.mcts._tree)
    assert torch.equal(eager.mcts.principal_variations(), graph.mcts.principal_variations())
    assert all(torch.equal(a, b) for a, b in zip(eager.mcts.root_visits(), graph.mcts.root_visits()))
    assert torch.equal(eager.env.current().observations, graph.env.current().observations)


def test_set_mcts_rewrites_the_table_under_the_same_graph():
    arena, fresh, plain = _arena(True, seed=31, mcts=CTL), _arena(True, seed=31, mcts=CTL), _arena(True, seed=31)
    r0, s0 = arena.run_round(PAIRINGS, games_per_match=4)
    graph, table = arena._graph, arena.ply.stages["mcts"].table
    assert graph is not None and s0.mcts.simulations > 2 * s0.mcts.searched
    arena.set_mcts(ONE)
    assert table[:, 3].tolist() == [1, 1]
    r1, s1 = arena.run_round(PAIRINGS, games_per_match=4)
    assert s1.mcts.simulations == s1.mcts.searched > 100 and s1.mcts.revisits == 0     # one simulation: the top logit is played
    arena.set_mcts(None)                                      # every row off: the games of an arena without a search
    r3, s3 = arena.run_round(PAIRINGS, games_per_match=4)
    p3, t3 = plain.run_round(PAIRINGS, games_per_match=4)
    assert s3.mcts == type(s3.mcts)() and t3.mcts is None and _key(r3) == _key(p3) and _games(r3) == _games(p3)
    arena.set_mcts(CTL)
    assert arena._graph is graph and arena.ply.stages["mcts"].table is table and table[:, 3].tolist() == [6, 2]
    r2, s2 = arena.run_round(PAIRINGS, games_per_match=4)
    f0, _ = fresh.run_round(PAIRINGS, games_per_match=4)      # the rounds depend on the table alone
    fresh.set_mcts(ONE)
    f1, _ = fresh.run_round(PAIRINGS, games_per_match=4)
    fresh.set_mcts(CTL)
    f2, t2 = fresh.run_round(PAIRINGS, games_per_match=4)
    assert _games(f0) == _games(r0) and _games(f1) == _games(r1) and _games(f2) == _games(r2) and t2.mcts == s2.mcts
    assert _games(r1) != _games(r0) and _games(r3) != _games(r0)


def test_mcts_none_leaves_the_ply_record_what_it_was():
    kw = dict(sync_every=2, graph=False, seed=22, record=True)
    none = MatchArena(_group(), N, PER, MAX_PLY, mcts=None, **kw)
    plain = MatchArena(_group(), N, PER, MAX_PLY, **kw)
    assert none.mcts is None and "mcts" not in none.ply.stages and none.ply.mcts is None
    r0, s0 = none.run_round(PAIRINGS, games_per_match=2)
    r1, s1 = plain.run_round(PAIRINGS, games_per_match=2)
    assert _key(r0) == _key(r1) and s0.mcts is None and len(none.record) == len(plain.record) >= 10
    for a, b in zip(none.record, plain.record):
        assert a.keys() == b.keys() and not any(k.startswith("mcts") or k.startswith("node_") for k in a)
        assert all(torch.equal(a[k], b[k]) if isinstance(a[k], torch.Tensor) else a[k] == b[k] for k in a)
    # every row off: nothing is allocated and nothing is launched
    off = MatchArena(_group(), N, PER, MAX_PLY, mcts=MctsControls.OFF, **kw)
    assert off.mcts is None and off.ply.stages["mcts"].table is not None
    r2, s2 = off.run_round(PAIRINGS, games_per_match=2)
    assert _key(r2) == _key(r0) and s2.mcts == type(s2.mcts)()
    assert all(torch.equal(a["actions"], b["actions"]) for a, b in zip(off.record, none.record))


def test_a_mate_behind_the_search_still_overrides():
    """Games started from mate-in-one positions: model 0 searches and has the mate check behind the search, model 1 only
    searches -- at width 1, so that the search's choice is the top logit and the mate is hardly ever it.  Every game model 0
    moves first in is won at once, whatever the visits said."""
    def arena(mate):
        a = MatchArena(_group(), N, PER, 40, sync_every=2, graph=True, seed=17, game_log=256, start_pool_capacity=16,
                       mcts=[MctsControls(1, 2, 1.25)] * 2, mate=mate)
        a.env.set_start_sfens(MH.pool_sfens(), seed=5)
        return a
    results, stats = arena([MateControls(16), MateControls.OFF]).run_round([(0, 1), (1, 0)], games_per_match=8)
    first = lambda g: g.black if g.start_side == 0 else g.white  # noqa: E731
    mine = [g for r in results for g in r.recorded_games if not g.carried and first(g) == 0]
    assert len(mine) >= 4 and stats.mate.mates >= len(mine) and stats.mcts.searched > 0
    for g in mine:
        assert len(g.actions) == 1 and g.reason == 1 and g.winner == g.start_side, (g.env, g.actions)
    assert stats.mate.changed >= 1                            # and at least once the mate was not the search's choice


def test_refusals():
    la, se = [LookaheadControls(3, 0.25)] * 2, [SearchControls(3, 4)] * 2
    with pytest.raises(ValueError, match="cannot be combined with lookahead="):
        MatchArena(_group(), N, PER, MAX_PLY, graph=False, mcts=CTL, lookahead=la)
    with pytest.raises(ValueError, match="cannot be combined with search="):
        MatchArena(_group(), N, PER, MAX_PLY, graph=False, mcts=CTL, search=se)
    with pytest.raises(ValueError, match="cannot be combined with collect=True"):
        MatchArena(_group(), N, PER, MAX_PLY, graph=False, mcts=CTL, collect=True)
    arena = MatchArena(_group(), N, PER, MAX_PLY, graph=False, mcts=CTL)
    with pytest.raises(ValueError, match="above the width"):
        arena.set_mcts(MctsControls(4, 2))
    with pytest.raises(ValueError, match="above the simulations"):
        arena.set_mcts(MctsControls(3, 7))
    arena.set_mcts(MctsControls(3, 6))
    with pytest.raises(ValueError, match="built without mcts="):
        MatchArena(_group(), N, PER, MAX_PLY, graph=False).set_mcts(CTL)
    env = VecEnv(4, 24, "katago", "spatial", output="torch", check_actions=True)
    env.reset()
    with pytest.raises(ValueError, match="simulations must be an integer"):
        MctsSearch(env, _group(), 3, 65)
    with pytest.raises(ValueError, match="width must be an integer"):
        MctsSearch(env, _group(), 0, 2)
    ms = MctsSearch(env, _group(), 3, 2)
    with pytest.raises(ValueError, match="simulation 2 lies outside"):
        ms.records(2)
    t = _table(MctsControls(3, 2))
    with pytest.raises(_lib.KeiseiHipError, match="simulation must lie in"):
        _lib.call("ka_mcts_advance", ms._records, ms._tree, 3, 2, 2, t, ms.active, 1, ms.value_logits, ms.rewards,
                  ms.terminated, ms.truncated, ms._step_err, ms.actions, ms.parent_row, ms.active, ms._pv, ms._root_visits,
                  ms._root_values, ms._counters, ms._counters, 4, _stream())
    with pytest.raises(_lib.KeiseiHipError, match="simulations must lie in"):
        _lib.call("ka_mcts_advance", ms._records, ms._tree, 3, 65, 0, t, ms.active, 1, ms.value_logits, ms.rewards,
                  ms.terminated, ms.truncated, ms._step_err, ms.actions, ms.parent_row, ms.active, ms._pv, ms._root_visits,
                  ms._root_values, ms._counters, ms._counters, 4, _stream())
