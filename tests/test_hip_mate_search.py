"""csrc/mate.hip behind VecEnv.mate_in_one and MateSearch against the C oracle, move for move: the checking moves of every
position in ascending action order, the cap, the mate the env step finds among them, and an env that is only read."""
import numpy as np
import pytest
import torch

import mate_search_helpers as H
from keisei_amd import _lib
from keisei_amd.shogi_gym import ACTION_SPACE, MASK_WORDS, VecEnv
from keisei_amd.training import MateControls, MateSearch, mate_table
from keisei_amd.training.mate_search import (FLAG_ACTIVE, FLAG_CHANGED, FLAG_MATE, FLAG_TRUNCATED, REC_ACTION, REC_FLAGS,
                                             REC_LIST, REC_NCHECKS, REC_SLOT)
from oracle.shogi import OracleVecEnv

pytestmark = pytest.mark.gpu
DEV = "cuda"
N = 13


def _loaded(max_ply=200):
    """One env per helper position (13 of them; any remainder would be the start position)."""
    env = VecEnv(N, max_ply, "katago", "spatial")
    env.reset()
    names = list(H.NAMES) + ["start"] * (N - len(H.NAMES))
    pos = [H.position(n) for n in names]
    env.set_states(np.stack([p[0] for p in pos]), np.stack([p[1] for p in pos]), np.array([p[2] for p in pos], np.uint8))
    return env, names


def _compare(env, cap, expect, tag=""):
    """``mate_in_one(cap)`` and its records against ``expect`` = per env (checks, mates) of the oracle."""
    actions, n_checks, truncated = env.mate_in_one(max_checks=cap)
    rec = env.mate_records(cap).cpu().numpy()
    assert actions.dtype == n_checks.dtype == truncated.dtype == torch.int64 and actions.shape == (env.num_envs,)
    actions, n_checks, truncated = actions.cpu().numpy(), n_checks.cpu().numpy(), truncated.cpu().numpy()
    assert rec.shape == (env.num_envs, 4 + cap)
    for e, (checks, mates) in enumerate(expect):
        forked, trunc, mate = H.expected_record(checks, mates, cap)
        where = f"{tag} env {e} cap {cap}"
        assert n_checks[e] == len(checks), (where, int(n_checks[e]), len(checks))
        assert rec[e, REC_LIST:].tolist() == forked + [-1] * (cap - len(forked)), (where, rec[e, REC_LIST:].tolist(), forked)
        assert bool(truncated[e]) == trunc, where
        assert actions[e] == mate, (where, int(actions[e]), mate)
        flags = int(rec[e, REC_FLAGS])
        assert bool(flags & FLAG_ACTIVE) == (len(checks) > 0) and bool(flags & FLAG_MATE) == (mate >= 0), (where, flags)
        assert bool(flags & FLAG_TRUNCATED) == trunc and rec[e, REC_NCHECKS] == len(checks), where
        if mate >= 0:
            assert rec[e, REC_LIST + rec[e, REC_SLOT]] == mate == rec[e, REC_ACTION], where
        else:
            assert rec[e, REC_SLOT] == -1, where
    return actions, n_checks, truncated


def test_positions_checking_moves_and_mates_equal_the_oracle():
    env, names = _loaded()
    expect = [H.expected(n) for n in names]
    actions, n_checks, _ = _compare(env, 64, expect)
    for e, n in enumerate(names):                              # the lowest-index oracle mate, or -1
        mates = H.expected(n)[1]
        assert actions[e] == (mates[0] if mates else -1), n
    assert (actions >= 0).sum() == len(H.WITH_MATE) + 1 and n_checks[names.index("start")] == 0


@pytest.mark.parametrize("cap", [4, 16])
def test_cap_cuts_the_list_and_sets_truncated(cap):
    env, names = _loaded()
    expect = [H.expected(n) for n in names]
    actions, n_checks, truncated = _compare(env, cap, expect)
    assert truncated.tolist() == [int(len(c) > cap) for c, _ in expect] and truncated.sum() >= 3
    o = names.index("open")
    assert actions[o] == -1 and truncated[o] == 1              # the mate lies behind the first 16 checking moves
    if cap == 16:
        again = env.mate_in_one(max_checks=64)
        assert again[0][o].item() == H.expected("open")[1][0] and again[2][o].item() == 0


def _search(env, cap=16):
    return MateSearch(env, cap), _lib.stream_ptr(torch.device(DEV))


def _table(controls, K=1):
    return torch.from_numpy(mate_table(controls, K)).to(DEV)


def test_an_incoming_mate_is_kept_and_inactive_envs_keep_their_actions():
    env = VecEnv(2, 200, "katago", "spatial")
    env.reset()
    board, hands, side = H.position("gold_head")
    env.set_states(np.stack([board] * 2), np.stack([hands] * 2), np.array([side] * 2, np.uint8))
    checks, mates = H.expected("gold_head")
    assert len(mates) >= 2
    search, st = _search(env)
    bits = env._bits[env._cur]
    first_legal = int(env._mask[env._cur][1].to(torch.uint8).argmax())
    incoming = torch.tensor([mates[1], first_legal], dtype=torch.int64, device=DEV)        # env 0: a mate, not the lowest
    # env 1 has no model: only env 0 is looked at, and its action stays
    actions = incoming.clone()
    search.clear()
    search.step(bits, actions, torch.tensor([0, -1], dtype=torch.int32, device=DEV), _table(MateControls(16)), st)
    stats = search.read()
    assert torch.equal(actions, incoming)
    assert (stats.positions, stats.forked, stats.mates, stats.changed, stats.truncated) == (1, len(checks), 1, 0, 0)
    rec = search.records().cpu().numpy()
    assert rec[0, REC_FLAGS] == FLAG_ACTIVE | FLAG_MATE and rec[0, REC_ACTION] == mates[1]
    assert rec[0, REC_LIST + rec[0, REC_SLOT]] == mates[1] and rec[1, REC_FLAGS] == 0 and rec[1, REC_ACTION] == first_legal
    # both envs on, env 1's action is no mate: it becomes the lowest one
    actions = incoming.clone()
    search.clear()
    search.step(bits, actions, torch.zeros(2, dtype=torch.int32, device=DEV), _table(MateControls(16)), st)
    stats = search.read()
    assert actions.tolist() == [mates[1], mates[0]] and (stats.mates, stats.changed) == (2, 1)
    assert search.records()[1, REC_FLAGS].item() == FLAG_ACTIVE | FLAG_MATE | FLAG_CHANGED
    # a row that is off, rows outside the ranges, a model outside the table, skip_plies above the game ply (0 here)
    off = [_table(MateControls.OFF), _table(MateControls(16, 1)),
           torch.tensor([[65, 0, 0, 0]], dtype=torch.int32, device=DEV), torch.tensor([[-1, 0, 0, 0]], dtype=torch.int32, device=DEV),
           torch.tensor([[16, -1, 0, 0]], dtype=torch.int32, device=DEV)]
    for table, model in [(t, 0) for t in off] + [(_table(MateControls(16)), -1), (_table(MateControls(16)), 1)]:
        actions = incoming.clone()
        search.clear()
        search.step(bits, actions, torch.full((2,), model, dtype=torch.int32, device=DEV), table, st)
        assert torch.equal(actions, incoming), (table.tolist(), model)
        assert search.read() == type(stats)() and (search.records()[:, REC_FLAGS] == 0).all()
    # max_checks below the cap cuts the list: the first checking move alone is no mate here
    assert mates[0] != checks[0]
    actions = incoming.clone()
    search.clear()
    search.step(bits, actions, torch.zeros(2, dtype=torch.int32, device=DEV), _table(MateControls(1)), st)
    assert torch.equal(actions, incoming) and search.read().truncated == 2
    assert search.records()[0, REC_LIST:].tolist() == [checks[0]] + [-1] * 15


def test_the_env_is_only_read_and_the_answer_repeats():
    env, _ = _loaded()
    watched = lambda: [t.clone() for t in (env._state, env._keys, env._checks, env._mask[env._cur], env._bits[env._cur],  # noqa: E731
                                           env._obs[env._cur], env._err, env._stats, env._rewards[env._cur])]
    before, cur = watched(), env._cur
    first = env.mate_in_one(max_checks=64)
    second = env.mate_in_one(max_checks=64)
    assert env._cur == cur and all(torch.equal(a, b) for a, b in zip(before, watched()))
    assert all(torch.equal(a, b) for a, b in zip(first, second))
    env.raise_if_refused()


def test_a_playout_in_lockstep_with_the_oracle():
    n, plies, max_ply, seed = 32, 48, 200, 3
    dev, ref = VecEnv(n, max_ply, "katago", "spatial"), OracleVecEnv(n, max_ply)
    dev.reset()
    _, mask = ref.reset()
    rng = np.random.default_rng(seed)
    with_check = with_mate = 0
    for t in range(plies):
        # only then is the history-free definition of the helpers exact: no move of this ply can complete a fourth repetition
        assert max(ref.repetition_count(i) for i in range(n)) < 3, t
        expect = []
        for i in range(n):
            board, hands, side, ply = ref.state(i)
            checks, mates, legal = H.oracle_checks(board, hands, side)
            assert np.array_equal(legal, mask[i])
            expect.append((checks, mates))
        with_check += sum(bool(c) for c, _ in expect)
        with_mate += sum(bool(m) for _, m in expect)
        _compare(dev, 64, expect, tag=f"ply {t}")
        acts = np.array([rng.choice(np.flatnonzero(m)) for m in mask], dtype=np.int64)
        rd, rr = dev.step(acts), ref.step(acts)
        assert np.array_equal(rd.legal_masks, rr["legal_masks"]) and np.array_equal(rd.terminated, rr["terminated"])
        mask = rr["legal_masks"]
    assert with_check >= 1 and with_mate >= 1                  # (seed 3: 344 positions with a checking move, 2 with a mate)
    assert int(dev._state[:, 100:104].contiguous().view(torch.int32).max()) >= 40              # long histories were copied


@pytest.mark.parametrize("which", ["even", "odd"])
@pytest.mark.parametrize("max_ply", [24, 23, 16])          # (history rows copied in 16-byte, 8-byte and single-byte pieces)
def test_forked_rows_at_every_history_width_are_the_replayed_games(max_ply, which):
    """The fork copy with a history behind every env: a scripted line ends at ply 6 (even) or 5 (odd) with at least one
    checking move, and the key rows go in 16-byte (24, 16) or 8-byte (23) pieces, the check rows in 4-byte (24), single-byte (23) or
    16-byte (16) pieces."""
    acts, expect = H.line(which)
    plies, n = acts.shape
    assert plies >= 5 and plies % 2 == (which == "odd") and all(len(checks) >= 1 for checks, _ in expect)
    cap = 4
    env = VecEnv(n, max_ply, "katago", "spatial")
    env.reset()
    for a in acts:
        env.step(a)
    search, st = _search(env, cap)
    bits = env._bits[env._cur]
    incoming = env._mask[env._cur].to(torch.uint8).argmax(dim=1)
    search.fork(bits, incoming.clone(), torch.zeros(n, dtype=torch.int32, device=DEV), _table(MateControls(cap)), st)
    torch.cuda.synchronize()
    lists = search._records[:, REC_LIST:].cpu().numpy()
    used = torch.from_numpy((lists >= 0).reshape(-1)).to(DEV)
    assert lists.tolist() == [list(checks[:cap]) + [-1] * (cap - len(checks[:cap])) for checks, _ in expect]
    rows = lambda t: t.repeat_interleave(cap, dim=0)  # noqa: E731
    assert int(env._state[:, 100:104].contiguous().view(torch.int32).min()) == plies
    assert torch.equal(search.child_state, rows(env._state)) and torch.equal(search.child_bits_in, rows(bits))
    assert torch.equal(search.child_keys[used, :plies], rows(env._keys)[used, :plies])
    assert torch.equal(search.child_checks[used, :plies], rows(env._checks)[used, :plies])
    assert bool(env._keys[:, :plies].ne(0).all()) and torch.equal(search.child_actions[used].cpu(),
                                                                  torch.from_numpy(lists.reshape(-1)[lists.reshape(-1) >= 0]))
    search.step_children(st)
    torch.cuda.synchronize()
    assert not bool(search._child_err.any())
    # a second VecEnv of n * cap rows: row e * cap + j replays env e's line, then plays what slot j plays
    rep = VecEnv(n * cap, max_ply, "katago", "spatial", output="torch", check_actions=True)
    rep.reset()
    for a in acts:
        rep.step(torch.from_numpy(a).to(DEV).repeat_interleave(cap))
    r = rep.step(search.child_actions.clone())
    for name, got, want in (("state", search.child_state, rep._state), ("keys", search.child_keys[:, :plies + 1], rep._keys[:, :plies + 1]),
                            ("checks", search.child_checks[:, :plies + 1], rep._checks[:, :plies + 1]),
                            ("observation", search.child_obs, r.observations), ("packed mask", search.child_mask_bits, r.legal_mask_bits),
                            ("reward", search.child_rewards, r.rewards), ("terminated", search.child_terminated, r.terminated),
                            ("truncated", search.child_truncated, r.truncated),
                            ("termination reason", search.child_reason, r.step_metadata.termination_reason),
                            ("current player", search.child_players, r.current_players)):
        assert got.dtype == want.dtype and torch.equal(got[used], want[used]), name


def test_refused_calls():
    env, _ = _loaded()
    search, st = _search(env, 4)
    bits, table = env._bits[env._cur], _table(MateControls(4))
    actions, model_of = torch.zeros(N, dtype=torch.int64, device=DEV), torch.zeros(N, dtype=torch.int32, device=DEV)

    def fork(**kw):
        a = dict(legal=bits, words=MASK_WORDS, actions=actions, model_of=model_of, K=1, table=table, cap=4, A=ACTION_SPACE)
        a.update(kw)
        _lib.call("ka_mate_fork", a["legal"], a["words"], a["actions"], a["model_of"], a["K"], a["table"], env._state, env._keys,
                  env._checks, env._max_ply, a["cap"], search._records, search.child_state, search.child_keys,
                  search.child_checks, search.child_bits_in, search.child_actions, N, a["A"], st)

    fork()
    for kw, text in ((dict(legal=None), "null"), (dict(table=None), "null"), (dict(words=MASK_WORDS - 1), "mask rows"),
                     (dict(A=ACTION_SPACE - 1), "spatial"), (dict(cap=0), "cap"), (dict(cap=65), "cap"), (dict(K=0), "at least one row"),
                     (dict(table=table.data_ptr() + 2), "table")):
        with pytest.raises(_lib.KeiseiHipError, match=text):
            fork(**kw)
    with pytest.raises(_lib.KeiseiHipError, match="cap"):
        _lib.call("ka_mate_choose", search._records, 65, search.child_rewards, search.child_terminated, search.child_reason,
                  search._child_err, actions, search._counters, search._counters.data_ptr() + 20, N, st)
    with pytest.raises(_lib.KeiseiHipError, match="null"):
        _lib.call("ka_mate_choose", None, 4, search.child_rewards, search.child_terminated, search.child_reason,
                  search._child_err, actions, search._counters, search._counters.data_ptr() + 20, N, st)
    with pytest.raises(ValueError, match="katago"):
        VecEnv(2, 50).mate_in_one()
    with pytest.raises(ValueError, match="max_checks"):
        env.mate_in_one(max_checks=0)
    with pytest.raises(ValueError, match="cap"):
        MateSearch(env, 65)
