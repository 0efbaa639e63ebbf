"""csrc/mate3.hip behind VecEnv.mate_in_three and Mate3Search against the C oracle, record for record: the evasion counts of
every check, the budget walk's rows, the proving set, the choice and the three cut flags, on the hand-built positions at the
caps that cut each of them, over a lockstep playout with histories behind every position, and ka_mate3_choose alone on
hand-made buffers for the rules no position was found for."""
import numpy as np
import pytest
import torch

import mate3_helpers as M
import mate_search_helpers as H
from keisei_amd import _lib
from keisei_amd.shogi_gym import VecEnv
from keisei_amd.training.mate_search import (ERR3_GRAND_STEP, FLAG3_ACTIVE, FLAG3_CHANGED, FLAG3_MATE, FLAG3_REPLY_TRUNCATED,
                                             FLAG_ACTIVE, FLAG_MATE, REC3_ACTION, REC3_FLAGS, REC3_PROVING, REC3_SLOT,
                                             REC_LIST, Mate3Stats, mate3_words, mate_words)
from oracle.shogi import OracleVecEnv

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAX_PLY = 64
# the default caps; what finds `late`; the root cut; the third-ply cut; the budget cut; everything `interpose` needs
CAPS = [(16, 32, 8), (16, 64, 16), (8, 64, 16), (16, 64, 8), (16, 32, 16), (64, 128, 64)]
_ENVS = {}


def _loaded(names):
    """One env per named position, built once per set of names: the probe only reads it."""
    if names not in _ENVS:
        env = VecEnv(len(names), MAX_PLY, "katago", "spatial")
        env.reset()
        pos = [M.position(n) if n in M.POSITIONS else H.position(n) for n in names]
        env.set_states(np.stack([p[0] for p in pos]), np.stack([p[1] for p in pos]), np.array([p[2] for p in pos], np.uint8))
        _ENVS[names] = env
    return _ENVS[names]


def _compare(env, caps, expect, tag=""):
    """``mate_in_three(*caps)``, its records and its counters against ``expect`` = per env the oracle's ``Expected3``."""
    cap = caps[0]
    incoming = env._mask[env._cur].to(torch.uint8).argmax(dim=1).cpu().numpy()      # what the probe hands in: the first legal move
    move, depth, cut = env.mate_in_three(*caps)
    root, deep = (r.cpu().numpy() for r in env.mate3_records(*caps))
    stats = env._mate[tuple(caps)][0].read()
    assert move.dtype == depth.dtype == cut.dtype == torch.int64 and move.shape == depth.shape == cut.shape == (env.num_envs,)
    assert root.shape == (env.num_envs, mate_words(cap)) and deep.shape == (env.num_envs, mate3_words(cap))
    move, depth, cut = move.cpu().numpy(), depth.cpu().numpy(), cut.cpu().numpy()
    for e, x in enumerate(expect):
        where = f"{tag} env {e} caps {caps}"
        assert root[e, REC_LIST:].tolist() == x.forked + [-1] * (cap - len(x.forked)), where
        assert bool(root[e, 0] & FLAG_ACTIVE) == bool(x.forked) and bool(root[e, 0] & FLAG_MATE) == (x.mate1 >= 0), where
        assert deep[e].tolist() == M.expected_words(x, cap, int(incoming[e])), (where, deep[e].tolist(), x)
        want = (x.mate1, 1) if x.mate1 >= 0 else (x.mate3, 3) if x.proving else (-1, 0)
        assert (int(move[e]), int(depth[e])) == want and bool(cut[e]) == x.cut, (where, int(move[e]), int(depth[e]), int(cut[e]))
    assert stats == Mate3Stats(sum(x.active for x in expect), sum(x.rows for x in expect), sum(x.reply_rows for x in expect),
                               sum(bool(x.proving) for x in expect),
                               sum(bool(x.proving) and x.choice(int(a)) != a for x, a in zip(expect, incoming)),
                               sum(x.skipped for x in expect)), (tag, caps, stats)
    return move, depth, cut


@pytest.mark.parametrize("caps", CAPS)
def test_named_positions_and_their_mirrors_equal_the_oracle(caps):
    env = _loaded(M.NAMES)
    expect = [M.expected(n, *caps) for n in M.NAMES]
    move, depth, cut = _compare(env, caps, expect)
    at = M.NAMES.index
    for tail in ("", "_white"):
        assert (move[at("simple" + tail)], depth[at("simple" + tail)]) == (2499, 3)
        assert move[at("two_ways" + tail)] == 3610 and depth[at("none" + tail)] == 0 == depth[at("pawn_drop3" + tail)]
        late, inter = at("late" + tail), at("interpose" + tail)
        assert (move[late], depth[late]) == ((5423, 3) if caps in ((16, 64, 16), (64, 128, 64)) else (-1, 0))
        assert cut[late] == (caps not in ((16, 64, 16), (64, 128, 64)))
        assert (move[inter], depth[inter], cut[inter]) == ((3613, 3, 0) if caps == (64, 128, 64) else (-1, 0, 1))


def test_the_mate_in_one_positions_stay_depth_one_with_the_move_mate_in_one_gives():
    env = _loaded(H.NAMES)
    expect = [M.expected3(*H.position(n), 64, 32, 8) for n in H.NAMES]
    move, depth, _ = _compare(env, (64, 32, 8), expect)
    one = env.mate_in_one(max_checks=64)[0].cpu().numpy()
    for e, n in enumerate(H.NAMES):
        if n in H.WITH_MATE or n == "open":
            assert depth[e] == 1 and move[e] == one[e] == H.expected(n)[1][0], n
        else:
            assert depth[e] != 1 and one[e] == -1, n


def test_an_incoming_proving_check_stays_and_a_row_out_of_range_has_depth_three_off():
    from keisei_amd.training.mate_search import Mate3Search, MateControls, mate3_reply_table, mate_table
    names = ("two_ways", "two_ways", "simple", "two_ways_white")
    env = _loaded(names)
    search, st = Mate3Search(env, 16, 32, 16), _lib.stream_ptr(torch.device(DEV))
    bits = env._bits[env._cur]
    first = int(env._mask[env._cur][2].to(torch.uint8).argmax())
    incoming = torch.tensor([3611, 3610, first, 3611], dtype=torch.int64, device=DEV)
    table = mate_table([MateControls(16, 0, 32, 16), MateControls(16)], 2)      # model 1 has the mate in one alone
    dev = lambda t: torch.from_numpy(t).to(DEV)  # noqa: E731
    actions = incoming.clone()
    search.clear()
    search.step(bits, actions, torch.tensor([0, 0, 0, 1], dtype=torch.int32, device=DEV), dev(table), dev(mate3_reply_table(table)), st)
    assert actions.tolist() == [3611, 3610, 2499, 3611]
    rec = search.records().cpu().numpy()
    assert rec[:3, REC3_FLAGS].tolist() == [FLAG3_ACTIVE | FLAG3_MATE] * 2 + [FLAG3_ACTIVE | FLAG3_MATE | FLAG3_CHANGED]
    assert rec[:3, REC3_SLOT].tolist() == [4, 3, 3] and rec[:2, REC3_PROVING].tolist() == [0b11000] * 2
    assert rec[3].tolist() == [0, 0, -1, 3611, 0, 0] + [-1] * 32           # the other model's env: its record says so
    x = M.expected("two_ways", 16, 32, 16)
    stats = search.read()
    assert stats == Mate3Stats(3, 2 * x.rows + 21, 2 * x.reply_rows + M.expected("simple", 16, 32, 16).reply_rows, 3, 1, 0)
    assert search.root.read().positions == 4                   # its mate in one looked at all four
    # words 2 / 3 outside their ranges: depth three is off, the mate in one is not
    for words in ([16, 0, 129, 16], [16, 0, -1, 16], [16, 0, 32, 65], [16, 0, 32, -1], [16, 0, 0, 0]):
        bad = np.array([words, words], np.int32)
        actions = incoming.clone()
        search.clear()
        search.step(bits, actions, torch.zeros(4, dtype=torch.int32, device=DEV), dev(bad), dev(mate3_reply_table(bad)), st)
        assert torch.equal(actions, incoming) and search.read() == Mate3Stats(), words
        assert (search.records()[:, REC3_FLAGS] == 0).all() and search.root.read().positions == 4


def test_the_env_is_only_read_and_the_answer_repeats():
    env = _loaded(M.NAMES)
    watched = lambda: [t.clone() for t in (env._state, env._keys, env._checks, env._mask[env._cur], env._bits[env._cur],  # noqa: E731
                                           env._obs[env._cur], env._err, env._stats, env._rewards[env._cur])]
    before, cur = watched(), env._cur
    first = env.mate_in_three(16, 64, 16)
    second = env.mate_in_three(16, 64, 16)
    assert env._cur == cur and all(torch.equal(a, b) for a, b in zip(before, watched()))
    assert all(torch.equal(a, b) for a, b in zip(first, second)) and (first[1] == 3).sum() == 6
    env.raise_if_refused()


# picked on the CPU with OracleVecEnv among seeds 0..11 (47 to 108 active positions): 108 of the 640 positions are active at
# depth three, with 940 grandchild rows, 1 974 third-ply rows, 3 skipped children and 11 third-ply cuts
PLAYOUT_SEED = 0


def test_a_playout_in_lockstep_with_the_oracle():
    n, plies, caps = 16, 40, (8, 32, 8)
    dev, ref = VecEnv(n, MAX_PLY, "katago", "spatial"), OracleVecEnv(n, MAX_PLY)
    dev.reset()
    _, mask = ref.reset()
    rng = np.random.default_rng(PLAYOUT_SEED)
    active = rows = 0
    for t in range(plies):
        # only then is the history-free definition of the helpers exact: no line of three plies can end by repetition or
        # at the move limit
        assert max(ref.repetition_count(i) for i in range(n)) < 3, t
        expect = []
        for i in range(n):
            board, hands, side, ply = ref.state(i)
            assert ply + 3 < MAX_PLY, (t, i, ply)
            expect.append(M.expected3(board, hands, side, *caps))
        active += sum(x.active for x in expect)
        rows += sum(x.rows for x in expect)
        _compare(dev, caps, expect, tag=f"ply {t}")
        acts = np.array([rng.choice(np.flatnonzero(m)) for m in mask], dtype=np.int64)
        rd, rr = dev.step(acts), ref.step(acts)
        assert np.array_equal(rd.legal_masks, rr["legal_masks"]) and np.array_equal(rd.terminated, rr["terminated"])
        mask = rr["legal_masks"]
    # a condition on the seed, checked on the CPU when it was picked: a playout without checks would prove nothing
    assert active >= 50 and rows >= 50, (active, rows)


@pytest.mark.parametrize("which", ["even", "odd"])
@pytest.mark.parametrize("max_ply", [24, 23, 16])          # (history rows copied in 16-byte, 8-byte and single-byte pieces)
def test_grandchild_rows_at_every_history_width_are_the_replayed_games(max_ply, which):
    """``Mate3Search.step`` behind a scripted line (ply 6 or 5; the children stand at ply 7 or 6 and stay open under every
    ceiling): every grandchild row in use is the replay of line + check + evasion -- the state, the first ply + 2 history
    entries, the mask, the reward and the done bytes."""
    from keisei_amd.training.mate_search import REC3_N, REC3_ROWS, Mate3Search, MateControls, mate3_reply_table, mate_table
    acts, expect = H.line(which)
    plies, n = acts.shape
    assert plies >= 5 and plies + 2 < max_ply and all(len(checks) >= 1 and not mates for checks, mates in expect)
    cap, rows, cap3 = 4, 32, 4
    env = VecEnv(n, max_ply, "katago", "spatial")
    env.reset()
    for a in acts:
        env.step(a)
    search, st = Mate3Search(env, cap, rows, cap3), _lib.stream_ptr(torch.device(DEV))
    table = mate_table(MateControls(cap, 0, rows, cap3), 1)
    incoming = env._mask[env._cur].to(torch.uint8).argmax(dim=1)
    actions = incoming.clone()
    search.clear()
    search.step(env._bits[env._cur], actions, torch.zeros(n, dtype=torch.int32, device=DEV), torch.from_numpy(table).to(DEV),
                torch.from_numpy(mate3_reply_table(table)).to(DEV), st)
    search.read()
    root, deep = search.root.records().cpu().numpy(), search.records().cpu().numpy()
    # per grandchild row: the check and the evasion that lead to it; a row not in use replays two fillers and is not compared
    check = incoming.cpu().numpy().repeat(rows)
    used = np.zeros(n * rows, bool)
    for e in range(n):
        assert deep[e, REC3_FLAGS] & FLAG3_ACTIVE and deep[e, REC3_ROWS] >= 1, e
        for j in range(cap):
            n_j, first = int(deep[e, REC3_N + j]), int(deep[e, REC3_N + cap + j])
            if first >= 0:
                check[e * rows + first:e * rows + first + n_j] = root[e, REC_LIST + j]
                used[e * rows + first:e * rows + first + n_j] = True
        assert used[e * rows:(e + 1) * rows].sum() == deep[e, REC3_ROWS], e
    rep = VecEnv(n * rows, max_ply, "katago", "spatial", output="torch", check_actions=True)
    rep.reset()
    for a in acts:
        rep.step(torch.from_numpy(a).to(DEV).repeat_interleave(rows))
    r = rep.step(torch.from_numpy(check).to(DEV))
    use = torch.from_numpy(used).to(DEV)
    assert not bool((r.terminated | r.truncated)[use].any())               # the children are open
    evasion = torch.where(use, search.grand_actions, r.legal_masks.to(torch.uint8).argmax(dim=1))
    # the rows in use of one check are its evasions: the set bits of the child's new mask, ascending
    for e in range(n):
        for j in range(cap):
            n_j, first = int(deep[e, REC3_N + j]), int(deep[e, REC3_N + cap + j])
            if first >= 0:
                legal = torch.nonzero(r.legal_masks[e * rows + first]).reshape(-1)
                assert torch.equal(search.grand_actions[e * rows + first:e * rows + first + n_j], legal), (e, j)
    r = rep.step(evasion)
    for name, got, want in (("state", search.grand_state, rep._state), ("keys", search.grand_keys[:, :plies + 2], rep._keys[:, :plies + 2]),
                            ("checks", search.grand_checks[:, :plies + 2], rep._checks[:, :plies + 2]),
                            ("packed mask", search.grand_mask_bits, r.legal_mask_bits), ("reward", search.grand_rewards, r.rewards),
                            ("terminated", search.grand_terminated, r.terminated), ("truncated", search.grand_truncated, r.truncated)):
        assert got.dtype == want.dtype and torch.equal(got[use], want[use]), name


# ---------------------------------------------------------------------------------------------- ka_mate3_choose alone
CAP, G, CAP3 = 4, 8, 2


def _buffers():
    """Five envs of three checks (actions 100, 200, 300) with rows 0-1, 2, 3-4: every grandchild open with a mate."""
    n = 5
    t = lambda a, dtype: torch.tensor(a, dtype=dtype, device=DEV)  # noqa: E731
    b = dict(n=n)
    b["rec1"] = t([[FLAG_ACTIVE, 3, -1, 7, 100, 200, 300, -1]] * n, torch.int32)
    b["rec"] = t([[FLAG3_ACTIVE, 5, -1, 7, 0, 0, 2, 1, 2, -1, 0, 2, 3, -1]] * n, torch.int32)
    rec3 = torch.zeros(n * G, mate_words(CAP3), dtype=torch.int32, device=DEV)
    rec3[:, 0] = FLAG_ACTIVE | FLAG_MATE
    rec3[:, 1] = 1
    b["rec3"] = rec3
    b["term"], b["trunc"] = torch.zeros(n * G, dtype=torch.bool, device=DEV), torch.zeros(n * G, dtype=torch.bool, device=DEV)
    b["err"] = [torch.zeros(2, dtype=torch.int64, device=DEV) for _ in range(3)]
    b["actions"] = t([7] * n, torch.int64)
    b["model_of"], b["table3"] = t([0] * n, torch.int32), t([[CAP3, 0, 0, 0]], torch.int32)
    b["counters"] = torch.zeros(7, dtype=torch.int32, device=DEV)
    return b


def _choose(b):
    _lib.call("ka_mate3_choose", b["rec"], b["rec1"], CAP, G, b["rec3"], CAP3, b["term"], b["trunc"], b["model_of"], 1,
              b["table3"], *b["err"], b["actions"], b["counters"], b["counters"].data_ptr() + 24, b["n"],
              _lib.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return b["rec"].cpu().numpy(), b["actions"].tolist(), b["counters"].tolist()


def test_choose_a_finished_grandchild_refutes_whatever_its_row_shows():
    b = _buffers()
    b["term"][0 * G + 1] = True                                # env 0: slot 0's second reply ended the game: a restarted
    b["trunc"][0 * G + 2] = True                               # row that "has a mate"; slot 1's reply was truncated
    b["actions"][1] = 300                                      # env 1: all three prove, the incoming one is the last
    b["rec"][2, 0] = 0                                         # env 2: not active at depth three
    b["rec3"][3 * G:3 * G + 5, 0] = FLAG_ACTIVE                # env 3: no reply runs into a mate;
    b["rec3"][3 * G + 3, 0] = FLAG_ACTIVE | 8                  # one of them with more checks than were forked
    b["rec3"][4 * G + 0, 0] = 0                                # env 4: a reply without any checking move refutes slot 0
    rec, actions, counters = _choose(b)
    assert actions == [300, 300, 7, 7, 200]
    assert rec[:, REC3_FLAGS].tolist() == [FLAG3_ACTIVE | FLAG3_MATE | FLAG3_CHANGED, FLAG3_ACTIVE | FLAG3_MATE, 0,
                                           FLAG3_ACTIVE | FLAG3_REPLY_TRUNCATED, FLAG3_ACTIVE | FLAG3_MATE | FLAG3_CHANGED]
    assert rec[:, REC3_PROVING].tolist() == [0b100, 0b111, 0, 0, 0b110] and (rec[:, REC3_PROVING + 1] == 0).all()
    assert rec[:, REC3_SLOT].tolist() == [2, 2, -1, -1, 1] and rec[:, REC3_ACTION].tolist() == [300, 300, 7, 7, 200]
    # positions, grandchild rows, third-ply rows (one per open row with a record, CAP3 for the truncated one), mates,
    # changed, skipped, then the error word
    assert counters == [4, 20, 3 + 5 + (4 + CAP3) + 4, 3, 2, 0, 0]


@pytest.mark.parametrize("which", [0, 1, 2])
def test_choose_a_refused_child_step_sets_the_error_bit_and_replaces_nothing(which):
    b = _buffers()
    b["err"][which][1] = 5
    before = b["rec"].clone()
    rec, actions, counters = _choose(b)
    assert actions == [7] * 5 and torch.equal(b["rec"], before)
    assert counters == [0, 0, 0, 0, 0, 0, 2 << which] and (2 << 1) == ERR3_GRAND_STEP


def test_refused_calls():
    from keisei_amd.training.mate_search import Mate3Search
    env = _loaded(M.NAMES)
    with pytest.raises(ValueError, match="rows"):
        Mate3Search(env, 16, 129, 8)
    with pytest.raises(ValueError, match="cap"):
        Mate3Search(env, 16, 32, 0)
    with pytest.raises(ValueError, match="positive"):
        env.mate_in_three(16, 0, 0)
    with pytest.raises(ValueError, match="both zero or both positive"):
        env.mate_in_three(16, 32, 0)
    with pytest.raises(ValueError, match="has not been called"):
        env.mate3_records(3, 3, 3)
    with pytest.raises(ValueError, match="katago"):
        VecEnv(2, 50).mate_in_three()
    b = _buffers()
    for kw, text in ((dict(cap=65), "cap"), (dict(G=129), "G in"), (dict(cap3=0), "cap3"), (dict(K=0), "at least one row")):
        a = dict(cap=CAP, G=G, cap3=CAP3, K=1)
        a.update(kw)
        with pytest.raises(_lib.KeiseiHipError, match=text):
            _lib.call("ka_mate3_choose", b["rec"], b["rec1"], a["cap"], a["G"], b["rec3"], a["cap3"], b["term"], b["trunc"],
                      b["model_of"], a["K"], b["table3"], *b["err"], b["actions"], b["counters"],
                      b["counters"].data_ptr() + 24, b["n"], _lib.stream_ptr(torch.device(DEV)))
    with pytest.raises(_lib.KeiseiHipError, match="null"):
        _lib.call("ka_mate3_gate", None, CAP, G, b["model_of"], b["rec3"], 352, b["term"], b["trunc"], b["model_of"],
                  b["actions"], 1, _lib.stream_ptr(torch.device(DEV)))
