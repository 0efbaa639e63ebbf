"""The reply search of the lookahead on the device: ka_lookahead_fork_replies / ka_lookahead_choose_replies against the float64
restatement, the forked grandchild rows against replayed games bit for bit, and MatchArena(lookahead=) with reply_width ply
by ply."""
import gc

import numpy as np
import pytest
import torch

from keisei_amd import _lib
from keisei_amd.shogi_gym import ACTION_SPACE, VecEnv
from keisei_amd.training import (Lookahead, LookaheadControls, MatchArena, lookahead_active, lookahead_candidates,
                                 lookahead_choose, lookahead_choose_replies, lookahead_reply_widths, lookahead_table)
from keisei_amd.training.lookahead import (FLAG_ACTIVE, FLAG_CHANGED, FLAG_REPLY_CHANGED, FLAG_WON, REC_ACTION, REC_CAND,
                                           REC_FLAGS, REC_NCAND, REC_SLOT)
from keisei_amd.training.model_group import SEResNetGroup
from keisei_amd.training.models.se_resnet import SEResNetModel, SEResNetParams
from oracle import keisei_oracle as orc
from oracle import shogi as S
from oracle.shogi import GOLD, KING, PAWN, WHITE, sq
from policy_insight_helpers import ATOL, RTOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPE = orc.NetShape(2, 128, 8, 64, 16, 128, 64)             # the smallest group the kernels accept: 128 channels, 2 blocks
_MODELS = []
_GROUP = {}


@pytest.fixture(autouse=True)
def _release_device_objects():
    """Arenas own captured graphs and pinned buffers: collect them with the device idle, not inside a later test's capture."""
    yield
    gc.collect()
    torch.cuda.synchronize()
    gc.collect()


def _group():
    if 2 not in _GROUP:
        while len(_MODELS) < 2:
            m = SEResNetModel(SEResNetParams(**SHAPE.__dict__))
            m.load_state_dict(orc.init_like_state_dict(SHAPE, salt=31 * len(_MODELS) + 7), strict=True)
            _MODELS.append(m.to(DEV).eval())
        _GROUP[2] = SEResNetGroup(_MODELS[:2])
    return _GROUP[2]


def _stream():
    return _lib.stream_ptr(torch.device(DEV))


def _unpack(bits: torch.Tensor) -> np.ndarray:
    j = np.arange(ACTION_SPACE)
    return ((bits.cpu().numpy().view(np.uint32)[:, j // 32] >> (j % 32).astype(np.uint32)) & 1).astype(bool)


def _table(*controls):
    return torch.from_numpy(lookahead_table(list(controls), len(controls))).to(DEV)


# ------------------------------------------------------------------ the scripted games
STEPS, WIDTH, REPLY = 14, 3, 3
MATE = S.encode(sq(1, 4), sq(1, 4), drop=GOLD)               # the gold drop on 5b
KING_HOME = S.encode(sq(0, 5), sq(0, 4), white=True)         # White's king back to 5a
_CACHE = {}


def _scripts(steps=STEPS):
    """Action histories of four envs, ``steps`` plies each (14, or 15 as tests/test_hip_lookahead.py plays them), checked move
    by move with the C oracle on the CPU, and per env the two moves that are interesting behind them.
    (a) four pawn moves, then both golds step up and back: the position after ply 4 stands again after plies 8 and 12; after 14
        plies Black's gold going home followed by White's gold going home makes it the fourth time;
    (b) pawn pushes only;
    (c) via set_state, White to move: king 5a, against a pawn on 5c, a gold in hand and a king walking along the ninth rank;
        after 14 plies the king going back to 5a allows the gold drop on 5b, which mates;
    (d) a bishop exchange and seeded legal moves: an ordinary middlegame."""
    if steps in _CACHE:
        return _CACHE[steps]
    a = [S.encode(sq(6, 2), sq(5, 2)), S.encode(sq(2, 6), sq(3, 6), white=True), S.encode(sq(6, 7), sq(5, 7)),
         S.encode(sq(2, 1), sq(3, 1), white=True)]
    cycle = [S.encode(sq(8, 5), sq(7, 5)), S.encode(sq(0, 3), sq(1, 3), white=True), S.encode(sq(7, 5), sq(8, 5)),
             S.encode(sq(1, 3), sq(0, 3), white=True)]
    a = (a + cycle * 3)[:16]
    b = [S.encode(sq(2, k // 2), sq(3, k // 2), white=True) if k % 2 else S.encode(sq(6, k // 2), sq(5, k // 2))
         for k in range(16)]
    c = []
    for k in range(15):
        if k % 2 == 0:
            f, t = (sq(0, 4), sq(0, 5)) if (k // 2) % 2 == 0 else (sq(0, 5), sq(0, 4))
            c.append(S.encode(f, t, white=True))
        else:
            c.append(S.encode(sq(8, k // 2), sq(8, k // 2 + 1)))
    c.append(MATE)
    assert c[14] == KING_HOME == 10441 and MATE == 1943
    board, hands = S.empty_board()
    board[sq(0, 4)], board[sq(2, 4)], board[sq(8, 0)] = KING | WHITE, PAWN, KING
    hands[0, GOLD - 1] = 1
    # (d) and the legality of everything: the oracle plays the scripts
    ref = S.OracleVecEnv(4, 24)
    _, mask = ref.reset()
    ref.set_state(2, board, hands, 1)
    mask[2] = ref.observe(2)[1]
    d = [S.encode(sq(6, 2), sq(5, 2)), S.encode(sq(2, 6), sq(3, 6), white=True), S.encode(sq(7, 1), sq(1, 7), promote=True),
         S.encode(sq(0, 6), sq(1, 7), white=True)]
    rng = np.random.default_rng(5)
    for k in range(16):
        if k >= len(d):
            d.append(int(rng.choice(np.flatnonzero(mask[3]))))
        acts = np.array([a[k], b[k], c[k], d[k]], dtype=np.int64)
        assert all(mask[i, acts[i]] for i in range(4)), (k, acts)
        r = ref.step(acts)
        if k < 15:
            assert not (r["terminated"] | r["truncated"]).any(), k
        mask = r["legal_masks"]
    # the facts the scenarios rest on, by the oracle: ply 16 is the fourth repetition in (a) and the mate in (c)
    assert r["terminated"][0] and r["termination_reason"][0] == S.R_REPETITION and r["rewards"][0] == 0.0
    assert r["terminated"][2] and r["termination_reason"][2] == S.R_CHECKMATE and r["rewards"][2] == 1.0
    assert not (r["terminated"][[1, 3]] | r["truncated"][[1, 3]]).any()
    hist = [a, b, c, d]
    out = ([h[:steps] for h in hist], (board, hands, 1), [h[steps] for h in hist], [h[steps + 1] for h in hist] if steps < 15 else None)
    _CACHE[steps] = out
    return out


def _craft(rng, legal_row: np.ndarray, first=None, third=None) -> torch.Tensor:
    """a logits row: noise in (-1, 0), and three legal moves at 3.0, 2.5 and 2.0 -- ``first`` / ``third`` where given"""
    row = torch.from_numpy(rng.uniform(-1.0, 0.0, ACTION_SPACE).astype(np.float32))
    legal = [int(x) for x in np.flatnonzero(legal_row)]
    for special in (first, third):
        assert special is None or legal_row[special]
    others = [x for x in legal if x not in (first, third)]
    top = [first if first is not None else others.pop(0), others.pop(0), third if third is not None else others.pop(0)]
    row[top[0]], row[top[1]], row[top[2]] = 3.0, 2.5, 2.0
    return row


def _scenario(max_ply, steps=STEPS):
    """a device VecEnv of 4 envs after the scripts, crafted root logits with the interesting move third, and the histories"""
    hist, start, move, reply = _scripts(steps)
    env = VecEnv(4, max_ply, "katago", "spatial", output="torch", check_actions=True)
    env.reset()
    env.set_state(2, *start)
    for k in range(steps):
        r = env.step(torch.tensor([h[k] for h in hist], dtype=torch.int64, device=DEV))
        assert not bool((r.terminated | r.truncated).any())
    masks = env.current().legal_masks.cpu().numpy()
    rng = np.random.default_rng(9)
    third = [move[0], None, move[2], None]
    logits = torch.stack([_craft(rng, masks[e], third=third[e]) for e in range(4)])
    return env, hist, start, logits.to(DEV), third, reply


def _two_plies(la, env, logits, model_of, table, craft_children=None):
    """fork, step, forward, (the child logits overwritten), reply fork, step, forward; returns the sampled actions"""
    cur = env.current()
    sampled = torch.tensor([int(np.flatnonzero(m)[0]) for m in cur.legal_masks.cpu().numpy()], dtype=torch.int64, device=DEV)
    la.clear()
    la.fork(logits, cur.legal_mask_bits, sampled, model_of, table, _stream())
    la.step_children(_stream())
    la.evaluate()
    if craft_children is not None:
        craft_children()
    la.fork_replies(table, _stream())
    la.step_grandchildren(_stream())
    la.evaluate_grandchildren()
    torch.cuda.synchronize()
    return sampled


def _lowest_legal(bits: torch.Tensor):
    return [int(np.flatnonzero(m)[0]) for m in _unpack(bits)]


# ------------------------------------------------------------------ 1. fork fidelity
@pytest.mark.parametrize("max_ply", [24, 23, 16, 15])      # (history rows copied in 16-byte, 8-byte and single-byte pieces)
def test_forked_grandchildren_are_the_replayed_games_bit_for_bit(max_ply):
    """The four scripted games after 14 plies, forked twice.  At max_ply 24 and 23 the fourth repetition of (a) and the mate
    of (c) happen in the grandchildren -- the repetition needs the key history through both forks; at 16 every grandchild is
    truncated; at 15 every child is, no child has replies, and the grandchild step must still not be refused."""
    env, hist, start, logits, third, reply = _scenario(max_ply)
    la = Lookahead(env, _group(), WIDTH, REPLY)
    table = _table(LookaheadControls(WIDTH, reply_width=REPLY))
    model_of = torch.zeros(4, dtype=torch.int32, device=DEV)
    rng = np.random.default_rng(10)

    def craft():                                              # the interesting reply third behind the interesting move
        if max_ply == 15:
            return
        masks = _unpack(la.child_mask_bits)
        for e in (0, 2):
            c = e * WIDTH + 2
            la.child_logits.reshape(-1, ACTION_SPACE)[c] = _craft(rng, masks[c], third=reply[e]).to(DEV)

    env_rows = (env._state, env._keys, env._checks, env.current().legal_mask_bits)
    before_env = [t.clone() for t in env_rows]
    _two_plies(la, env, logits, model_of, table, craft)
    child_rows = (la.child_state, la.child_keys, la.child_checks, la.child_mask_bits, la.child_obs, la.child_rewards,
                  la.child_terminated, la.child_truncated, la.child_logits, la.child_value_logits, la.child_model_of)
    # (the child rows are compared with what a second run of the first three stages and the overwrite leaves)
    before_child = [t.clone() for t in child_rows]
    la.fork_replies(table, _stream())
    la.step_grandchildren(_stream())
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(before_env, env_rows))        # the env's rows are only read
    assert all(torch.equal(x, y) for x, y in zip(before_child, child_rows))    # and so are the child rows
    assert not bool(la._child_err.any()) and not bool(la._grand_err.any())     # nothing was refused

    rec, rrec = la.records().cpu(), la.reply_records().cpu()
    cands = rec[:, REC_CAND:REC_CAND + WIDTH]
    assert rec[:, REC_NCAND].tolist() == [WIDTH] * 4 and cands[:, 2].tolist()[0] == third[0] and cands[2, 2] == KING_HOME
    live = ~(la.child_terminated | la.child_truncated).cpu()
    assert bool(live.all()) == (max_ply != 15) and bool(live.any()) == (max_ply != 15)
    # the replies are the restatement's candidates of the child logits over the children's own masks
    want_c, want_p, want_n = lookahead_candidates(la.child_logits.reshape(-1, ACTION_SPACE).cpu(), la.child_mask_bits.cpu(), REPLY)
    lowest = _lowest_legal(la.child_mask_bits)
    for c in range(4 * WIDTH):
        if live[c]:
            assert int(rrec[c, REC_FLAGS]) == FLAG_ACTIVE and int(rrec[c, REC_NCAND]) == int(want_n[c]) == REPLY, c
            assert rrec[c, REC_CAND:REC_CAND + REPLY].tolist() == want_c[c].tolist(), c
            np.testing.assert_allclose(rrec.view(torch.float32)[c, REC_CAND + REPLY:REC_CAND + 2 * REPLY].numpy().astype(np.float64),
                                       want_p[c].numpy(), rtol=RTOL, atol=ATOL)
            assert la.grand_actions[c * REPLY:(c + 1) * REPLY].cpu().tolist() == want_c[c].tolist()
            assert la.grand_model_of[c * REPLY:(c + 1) * REPLY].cpu().tolist() == [0] * REPLY
        else:
            assert int(rrec[c, REC_FLAGS]) == 0 and int(rrec[c, REC_NCAND]) == 0 and rrec[c, REC_CAND:REC_CAND + REPLY].eq(-1).all()
            assert la.grand_actions[c * REPLY:(c + 1) * REPLY].cpu().tolist() == [lowest[c]] * REPLY
            assert la.grand_model_of[c * REPLY:(c + 1) * REPLY].cpu().tolist() == [-1] * REPLY
    if max_ply != 15:
        assert int(rrec[0 * WIDTH + 2, REC_CAND + 2]) == reply[0] and int(rrec[2 * WIDTH + 2, REC_CAND + 2]) == MATE

    # a second env replays the history, then candidate j, then reply k
    G = 4 * WIDTH * REPLY
    rep = VecEnv(G, max_ply, "katago", "spatial", output="torch", check_actions=True)
    rep.reset()
    for g in range(2 * WIDTH * REPLY, 3 * WIDTH * REPLY):
        rep.set_state(g, *start)
    for k in range(STEPS):
        rep.step(torch.tensor([h[k] for h in hist], dtype=torch.int64, device=DEV).repeat_interleave(WIDTH * REPLY))
    rep.step(cands.reshape(-1).to(torch.int64).to(DEV).repeat_interleave(REPLY))
    r = rep.step(la.grand_actions.clone())
    for name, got, want in (("observation", la.grand_obs, r.observations), ("packed mask", la.grand_mask_bits, r.legal_mask_bits),
                            ("reward", la.grand_rewards, r.rewards), ("terminated", la.grand_terminated, r.terminated),
                            ("truncated", la.grand_truncated, r.truncated),
                            ("termination reason", la.grand_reason, r.step_metadata.termination_reason),
                            ("current player", la.grand_players, r.current_players)):
        assert got.dtype == want.dtype and torch.equal(got, want), name
    reason = la.grand_reason.cpu().numpy().reshape(4, WIDTH, REPLY)
    reward = la.grand_rewards.cpu().numpy().reshape(4, WIDTH, REPLY)
    if max_ply in (24, 23):
        assert reason[0, 2].tolist() == [S.R_PROGRESS, S.R_PROGRESS, S.R_REPETITION] and reward[0, 2, 2] == 0.0
        assert reason[2, 2].tolist() == [S.R_PROGRESS, S.R_PROGRESS, S.R_CHECKMATE] and reward[2, 2, 2] == 1.0
        assert (reason[:, :2] == S.R_PROGRESS).all() and (reason[[1, 3]] == S.R_PROGRESS).all()
    elif max_ply == 16:
        assert (reason == S.R_MAXMOVES).all() and bool(la.grand_truncated.all()) and not reward.any()
    else:
        assert (la.child_reason.cpu().numpy() == S.R_MAXMOVES).all() and bool(la.child_truncated.all())
        assert not bool((la.grand_terminated | la.grand_truncated).any())      # the first move of restarted games


# ------------------------------------------------------------------ 2. the blunder is refused
def _mating_replies():
    """by the C oracle: every (move, reply) of game (c) after 14 plies whose reply mates"""
    hist, start, _, _ = _scripts()

    def replay(n):
        ref = S.OracleVecEnv(n, 24)
        ref.reset()
        for i in range(n):
            ref.set_state(i, *start)
        for k in range(STEPS):
            r = ref.step(np.full(n, hist[2][k], dtype=np.int64))
        return ref, r["legal_masks"]

    _, mask = replay(1)
    moves = [int(x) for x in np.flatnonzero(mask[0])]
    ref, mask = replay(len(moves))
    r = ref.step(np.array(moves, dtype=np.int64))
    assert not (r["terminated"] | r["truncated"]).any()
    pairs = [(m, int(x)) for i, m in enumerate(moves) for x in np.flatnonzero(r["legal_masks"][i])]
    ref, _ = replay(len(pairs))
    ref.step(np.array([m for m, _ in pairs], dtype=np.int64))
    r = ref.step(np.array([x for _, x in pairs], dtype=np.int64))
    mates = [p for i, p in enumerate(pairs) if r["terminated"][i] and r["termination_reason"][i] == S.R_CHECKMATE]
    return moves, mates


def test_the_move_that_walks_into_a_mate_is_refused():
    moves, mates = _mating_replies()
    assert len(moves) == 4 and KING_HOME in moves and mates == [(KING_HOME, MATE)]
    env, hist, start, logits, _, _ = _scenario(24)
    W = 4
    la = Lookahead(env, _group(), W, REPLY)
    model_of = torch.zeros(4, dtype=torch.int32, device=DEV)
    masks = env.current().legal_masks.cpu().numpy()
    assert [int(x) for x in np.flatnonzero(masks[2])] == moves
    rng = np.random.default_rng(11)
    logits[2] = _craft(rng, masks[2], first=KING_HOME).to(DEV)
    c0 = 2 * W                                                # the child behind the king's move

    def craft():                                              # the mate is the third reply, and the value head likes the blunder
        la.child_logits.reshape(-1, ACTION_SPACE)[c0] = _craft(rng, _unpack(la.child_mask_bits[c0:c0 + 1])[0], third=MATE).to(DEV)
        la.child_value_logits[c0] = torch.tensor([-4.0, 0.0, 4.0], device=DEV)

    def run(reply_width):
        table = _table(LookaheadControls(W, 0.0, reply_width=reply_width))
        actions = _two_plies(la, env, logits, model_of, table, craft)
        sampled = actions.clone()
        la.choose_replies(actions, model_of, table, _stream())
        stats = la.read()
        return actions, sampled, stats, la.records().cpu(), la.reply_records().cpu()

    actions, sampled, stats, rec, rrec = run(3)
    f = rec.view(torch.float32)
    assert int(rec[2, REC_NCAND]) == 4 and int(rec[2, REC_CAND]) == KING_HOME
    assert rrec[c0, REC_CAND:REC_CAND + 3].tolist()[2] == MATE and int(rrec[c0, REC_SLOT]) == 2 and int(rrec[c0, REC_ACTION]) == MATE
    assert rrec.view(torch.float32)[c0, REC_CAND + 2 * REPLY + 2].item() == -1.0
    assert f[2, REC_CAND + 2 * W].item() == -1.0              # q of the blunder, exactly
    assert int(actions[2]) != KING_HOME and int(actions[2]) in moves and int(rec[2, REC_ACTION]) == int(actions[2])
    one = lookahead_choose(f[:, REC_CAND + W:REC_CAND + 2 * W].double(), rec[:, REC_NCAND], la.child_value_logits.cpu().reshape(4, W, 3),
                           la.child_rewards.cpu().reshape(4, W), (la.child_terminated | la.child_truncated).cpu().reshape(4, W), 0.0)
    assert int(one.slot[2]) == 0                              # the one-ply search plays the blunder
    assert int(rec[2, REC_FLAGS]) & FLAG_REPLY_CHANGED and stats.reply_changed >= 1 and stats.searched == 4
    assert stats.reply_changed == int((rec[:, REC_FLAGS] & FLAG_REPLY_CHANGED).ne(0).sum())
    r = env.step(actions)                                     # and the env accepts the move
    env.raise_if_refused()
    assert not bool(r.terminated[2])

    # with two replies the mate is not searched, and the record says so
    env, hist, start, logits2, _, _ = _scenario(24)
    la = Lookahead(env, _group(), W, REPLY)
    logits2[2] = logits[2]
    logits = logits2
    actions, sampled, stats, rec, rrec = run(2)
    assert int(rrec[c0, REC_NCAND]) == 2 and MATE not in rrec[c0, REC_CAND:REC_CAND + 3].tolist() and int(rrec[c0, REC_CAND + 2]) == -1
    assert rec.view(torch.float32)[2, REC_CAND + 2 * W].item() > -1.0
    assert la.grand_model_of[c0 * REPLY:(c0 + 1) * REPLY].cpu().tolist() == [0, 0, -1]


# ------------------------------------------------------------------ 3. inactive slots
def test_inactive_grandchild_slots_get_the_lowest_legal_action_and_no_model():
    """15 plies: in (c) the gold drop mates, so that child is done.  env 0: skipped (its ply 15 is below skip_plies), env 1: a
    model with reply_width 0, env 2: reply_width 3 with the mated child third, env 3: unseated."""
    env, hist, start, logits, third, _ = _scenario(24, steps=15)
    assert third[2] == MATE
    la = Lookahead(env, _group(), WIDTH, REPLY)
    ctl = [LookaheadControls(WIDTH, 0.1, reply_width=REPLY), LookaheadControls(WIDTH, 0.1), LookaheadControls(WIDTH, skip_plies=16, reply_width=REPLY)]
    table = _table(*ctl)
    model_of = torch.tensor([2, 1, 0, -1], dtype=torch.int32, device=DEV)
    sampled = _two_plies(la, env, logits, model_of, table)
    assert not bool(la._child_err.any()) and not bool(la._grand_err.any())     # the step is not refused
    rec, rrec = la.records().cpu(), la.reply_records().cpu()
    assert rec[:, REC_FLAGS].tolist() == [0, FLAG_ACTIVE, FLAG_ACTIVE, 0]
    assert la.child_model_of.cpu().tolist() == [-1] * 3 + [1] * 3 + [0] * 3 + [-1] * 3
    mated = 2 * WIDTH + 2
    assert bool(la.child_terminated[mated]) and float(la.child_rewards[mated]) == 1.0
    lowest = _lowest_legal(la.child_mask_bits)
    gm, ga = la.grand_model_of.cpu().reshape(-1, REPLY), la.grand_actions.cpu().reshape(-1, REPLY)
    for c in range(4 * WIDTH):
        has = c in (2 * WIDTH, 2 * WIDTH + 1)                 # the two live children of the model that searches replies
        assert bool(rrec[c, REC_FLAGS] & FLAG_ACTIVE) == has, c
        if has:
            n = int(rrec[c, REC_NCAND])
            assert 1 <= n <= REPLY and gm[c].tolist() == [0] * n + [-1] * (REPLY - n)
            assert ga[c].tolist() == rrec[c, REC_CAND:REC_CAND + n].tolist() + [lowest[c]] * (REPLY - n)
        else:
            assert gm[c].tolist() == [-1] * REPLY and ga[c].tolist() == [lowest[c]] * REPLY, c
            assert int(rrec[c, REC_ACTION]) == lowest[c] and int(rrec[c, REC_NCAND]) == 0
    # the env of the reply_width 0 model gets the record and action of ka_lookahead_choose, to the bit
    forked = la._records.clone()
    actions = sampled.clone()
    la.choose_replies(actions, model_of, table, _stream())
    stats = la.read()
    rec2 = la.records()
    la.clear()
    la._records.copy_(forked)
    plain = sampled.clone()
    la.choose(plain, model_of, table, _stream())
    one = la.read()
    rec1 = la.records()
    assert torch.equal(rec2[1], rec1[1]) and int(actions[1]) == int(plain[1])
    assert actions[[0, 3]].tolist() == sampled[[0, 3]].tolist() and torch.equal(rec2[[0, 3]], rec1[[0, 3]])
    # the mate in one is still taken: a done child keeps its reward
    assert int(actions[2]) == MATE and rec2.cpu().view(torch.float32)[2, REC_CAND + 2 * WIDTH + 2].item() == 1.0
    assert int(rec2[2, REC_FLAGS]) & FLAG_WON and (stats.searched, stats.won) == (2, 1) == (one.searched, one.won)
    assert one.reply_changed == 0


# ------------------------------------------------------------------ 4. the choice on synthetic inputs
def _triples(qs):
    return np.array([[np.log((0.8 - q) / 2), np.log(0.2), np.log((0.8 + q) / 2)] for q in qs], np.float32)


def _synthetic(B, width, R, seed):
    """rows whose u values differ by at least 1e-3 or not at all: the children's q come from five value-logit triples 0.3
    apart, the grandchildren's from five others whose |q| are all different and none of the children's (so that two values
    are equal only where they come from the same triple, or are rewards: -1, 0, 1), the priors are 0, 1/2 or 1 and the
    weight is 0.0371: different q lie at least 0.05 apart, the priors move u by 0.0371 at the most."""
    rng = np.random.default_rng(seed)
    vl = torch.from_numpy(_triples((-0.6, -0.3, 0.0, 0.3, 0.6))[rng.integers(0, 5, (B, width))])
    gv = torch.from_numpy(_triples((-0.45, -0.2, 0.1, 0.35, 0.5))[rng.integers(0, 5, (B, width, R))])
    done, gdone = torch.from_numpy(rng.random((B, width)) < 0.2), torch.from_numpy(rng.random((B, width, R)) < 0.2)
    rewards = torch.from_numpy(rng.integers(-1, 2, (B, width)).astype(np.float32)) * done
    grewards = torch.from_numpy(rng.integers(-1, 2, (B, width, R)).astype(np.float32)) * gdone
    priors = torch.from_numpy((rng.integers(0, 3, (B, width)) / 2).astype(np.float32))
    n_cand = torch.from_numpy(rng.integers(0, width + 1, B).astype(np.int32))
    n_cand[:4] = torch.tensor([0, 1, width, width])
    n_reply = torch.from_numpy(rng.integers(0, R + 1, (B, width)).astype(np.int32))
    return priors, n_cand, vl, rewards, done, n_reply, gv, grewards, gdone


@pytest.mark.parametrize("width,reply,weight", [(1, 1, 0.0), (3, 2, 0.0371), (8, 8, 0.0), (8, 8, 0.0371)])
def test_choose_replies_against_the_restatement(width, reply, weight):
    B = 600
    args = _synthetic(B, width, reply, 50 + width)
    want = lookahead_choose_replies(*args, weight)
    one = lookahead_choose(*args[:5], weight)
    for u in (want.u.numpy(), one.u.numpy()):                               # no row is ambiguous at either depth
        u = np.sort(u, axis=1)[:, ::-1]
        with np.errstate(invalid="ignore"):
            gaps = u[:, :-1] - u[:, 1:] if width > 1 else np.zeros((B, 0))
        gaps = gaps[np.isfinite(gaps)]
        assert ((gaps == 0) | (gaps >= 1e-3)).all()
        assert (gaps == 0).sum() >= 10 or width == 1
    got = lookahead_choose_replies(*(a.to(DEV) for a in args), weight)
    assert got.error == 0 and want.error == 0
    assert torch.equal(got.slot.cpu(), want.slot) and int((want.slot < 0).sum()) >= 1
    assert torch.equal(got.reply_slot.cpu(), want.reply_slot) and int((want.reply_slot >= 0).sum()) >= B // 8
    assert torch.equal(got.one_ply_slot.cpu(), want.one_ply_slot) and torch.equal(want.one_ply_slot, one.slot)
    assert torch.equal(got.reply_changed.cpu(), want.reply_changed) and (int(want.reply_changed.sum()) >= 10 or width == 1)
    used = (torch.arange(width)[None, :] < args[1][:, None]).numpy()
    np.testing.assert_allclose(got.q.cpu().numpy()[used], want.q.numpy()[used], rtol=RTOL, atol=ATOL)
    backed = (want.reply_slot >= 0).numpy()
    rused = backed[:, :, None] & (np.arange(reply)[None, None, :] < args[5].numpy()[:, :, None])
    np.testing.assert_allclose(got.v.cpu().numpy()[rused], want.v.numpy()[rused], rtol=RTOL, atol=ATOL)
    # rows without a single reply: the record of ka_lookahead_choose, to the bit
    none = list(args)
    none[5] = torch.zeros_like(args[5])
    zero = lookahead_choose_replies(*(a.to(DEV) for a in none), weight)
    plain = lookahead_choose(*(a.to(DEV) for a in args[:5]), weight)
    assert torch.equal(zero.slot, plain.slot) and torch.equal(zero.q, plain.q) and not bool(zero.reply_changed.any())


# ------------------------------------------------------------------ 5. the error bits
def test_the_three_error_bits_raise_from_read():
    env, hist, start, logits, _, _ = _scenario(24)
    la = Lookahead(env, _group(), WIDTH, REPLY)
    table = _table(LookaheadControls(WIDTH, reply_width=REPLY))
    model_of = torch.zeros(4, dtype=torch.int32, device=DEV)

    def run(poison=None):
        actions = _two_plies(la, env, logits, model_of, table)
        sampled = actions.clone()
        if poison is not None:
            poison()
        la.choose_replies(actions, model_of, table, _stream())
        return actions, sampled

    run()
    assert la.read().searched == 4

    def nan_in_a_live_grandchild():
        assert not bool(la.grand_terminated[1] | la.grand_truncated[1]) and int(la.grand_model_of[1]) == 0
        la.grand_value_logits[1, 2] = float("nan")
    run(nan_in_a_live_grandchild)
    with pytest.raises(RuntimeError, match="non-finite value logits"):
        la.read()
    assert np.isneginf(la.reply_records().cpu().view(torch.float32)[0, REC_CAND + 2 * REPLY + 1].item())
    assert np.isneginf(la.records().cpu().view(torch.float32)[0, REC_CAND + 2 * WIDTH].item())

    def nan_in_a_live_child():                                # its one-ply q is still computed
        la.child_value_logits[0, 0] = float("inf")
    run(nan_in_a_live_child)
    with pytest.raises(RuntimeError, match="non-finite value logits"):
        la.read()

    def refused_child_step():
        la._child_err[1] = (3 << 32) | 77
    actions, sampled = run(refused_child_step)
    assert torch.equal(actions, sampled)                      # nothing is chosen from children that did not move
    with pytest.raises(RuntimeError, match="child step refused"):
        la.read()

    def refused_grandchild_step():
        la._grand_err[1] = (5 << 32) | 78
    actions, sampled = run(refused_grandchild_step)
    assert torch.equal(actions, sampled)
    with pytest.raises(RuntimeError, match="grandchild step refused"):
        la.read()
    la.clear()
    assert la.read() == type(la.read())()


# ------------------------------------------------------------------ 6. - 10. the arena
N, PER, MAX_PLY = 8, 4, 20
PAIRINGS = [(0, 1), (1, 0), (1, 1)]                          # more pairings than slots, one model against itself
CTL = [LookaheadControls(3, 0.25, reply_width=2), LookaheadControls(2, 0.0, skip_plies=4, reply_width=0)]
ONE_PLY = [LookaheadControls(3, 0.25), LookaheadControls(2, 0.0, skip_plies=4)]
U24 = 2.0 ** -24                                              # the unit roundoff of fp32


def _u_bound(vls_a, vls_b, weight):
    """How far apart two u values must lie in float64 for the fp32 kernel to be held to their order: the bound of
    tests/test_hip_lookahead.py, (2 X + 13 + 2 w) u per candidate with u = 2^-24 and X the largest |logit - row maximum|, here
    with X taken over every value-logit triple behind the candidate -- its grandchildren's where q is backed up, its own
    otherwise.  A min moves by no more than its worst argument, taking it is exact, and 0 - x is exact."""
    def spread(vls):
        vls = [v for v in vls if np.isfinite(v).all()]
        return max([float(np.max(np.max(v) - v)) for v in vls], default=0.0)
    return ((2 * spread(vls_a) + 13 + 2 * weight) + (2 * spread(vls_b) + 13 + 2 * weight)) * U24


def test_every_recorded_arena_ply_is_the_restatement():
    grp = _group()
    arena = MatchArena(grp, N, PER, MAX_PLY, sync_every=2, graph=False, seed=21, record=True, lookahead=CTL)
    assert arena.ply.stages["lookahead"].engine.width == 3 and arena.ply.stages["lookahead"].engine.reply_width == 2
    results, stats = arena.run_round(PAIRINGS, games_per_match=4)
    recs = arena.record
    assert len(recs) >= 20 and stats.lookahead.searched > 100
    table = lookahead_table(CTL, 2)
    W, R = 3, 2
    active_rows = close_rows = changed = won = reply_changed = backed_children = done_grand = one_ply_rows = 0
    for t, rec in enumerate(recs):
        mo = rec["model_of"]
        logits = grp.forward(rec["obs"].to(DEV), mo.to(DEV), check=False).policy_logits.reshape(N, ACTION_SPACE).cpu()
        widths, weights = lookahead_active(table, mo, rec["game_plies"], width=W)
        rwidths = lookahead_reply_widths(table, mo, reply_width=R)
        cand, prior, n_cand = lookahead_candidates(logits, rec["mask_bits"], W)
        n_env = np.minimum(widths, n_cand.numpy())
        lr, rr = rec["lookahead_records"], rec["lookahead_reply_records"].reshape(N, W, -1)
        lf, rf = lr.view(torch.float32), rr.view(torch.float32)
        # the replies: the restatement's candidates of the recorded child logits over the children's masks
        rc, rp, rn = lookahead_candidates(rec["child_logits"], rec["child_mask_bits"], R)
        rc, rp, rn = rc.reshape(N, W, R), rp.reshape(N, W, R), rn.reshape(N, W)
        n_reply = torch.zeros(N, W, dtype=torch.int32)
        for e in range(N):
            for j in range(W):
                live = j < n_env[e] and not bool(rec["child_done"][e, j])
                n = min(int(rwidths[e]), int(rn[e, j])) if live else 0
                n_reply[e, j] = n
                assert bool(rr[e, j, REC_FLAGS] & FLAG_ACTIVE) == (n > 0) and int(rr[e, j, REC_NCAND]) == n, (t, e, j)
                assert rr[e, j, REC_CAND:REC_CAND + R].tolist() == rc[e, j, :n].tolist() + [-1] * (R - n), (t, e, j)
                np.testing.assert_allclose(rf[e, j, REC_CAND + R:REC_CAND + R + n].numpy().astype(np.float64), rp[e, j, :n].numpy(),
                                           rtol=RTOL, atol=ATOL)
        choice = lookahead_choose_replies(lf[:, REC_CAND + W:REC_CAND + 2 * W].double(), torch.from_numpy(n_env), rec["child_value_logits"],
                                          rec["child_rewards"], rec["child_done"], n_reply, rec["grand_value_logits"],
                                          rec["grand_rewards"], rec["grand_done"], torch.from_numpy(weights))
        assert choice.error == 0
        for e in range(N):
            n = int(n_env[e])
            flags = int(lr[e, REC_FLAGS])
            assert bool(flags & FLAG_ACTIVE) == (n > 0), (t, e)
            assert int(lr[e, REC_ACTION]) == int(rec["actions"][e]), (t, e)    # the stepped action is the recorded choice
            if n == 0:
                assert flags == 0 and int(lr[e, REC_NCAND]) == 0, (t, e)
                continue
            active_rows += 1
            one_ply_rows += int(rwidths[e] == 0)
            assert int(lr[e, REC_NCAND]) == n and lr[e, REC_CAND:REC_CAND + W].tolist() == cand[e, :n].tolist() + [-1] * (W - n), (t, e)
            np.testing.assert_allclose(lf[e, REC_CAND + 2 * W:REC_CAND + 2 * W + n].numpy().astype(np.float64),
                                       choice.q[e, :n].numpy(), rtol=RTOL, atol=ATOL)
            behind = []                                       # the value-logit triples behind every candidate
            for j in range(n):
                k = int(n_reply[e, j])
                backed_children += int(k > 0)
                done_grand += int(rec["grand_done"][e, j, :k].sum())
                if k:
                    np.testing.assert_allclose(rf[e, j, REC_CAND + 2 * R:REC_CAND + 2 * R + k].numpy().astype(np.float64),
                                               choice.v[e, j, :k].numpy(), rtol=RTOL, atol=ATOL)
                    behind.append([rec["grand_value_logits"][e, j, i].numpy().astype(np.float64) for i in range(k)
                                   if not bool(rec["grand_done"][e, j, i])])
                else:
                    behind.append([] if bool(rec["child_done"][e, j]) else [rec["child_value_logits"][e, j].numpy().astype(np.float64)])
            slot = int(lr[e, REC_SLOT])
            u = choice.u[e, :n].numpy()
            assert 0 <= slot < n and int(lr[e, REC_ACTION]) == int(lr[e, REC_CAND + slot]), (t, e)
            assert bool(flags & FLAG_WON) == (bool(rec["child_done"][e, slot]) and float(rec["child_rewards"][e, slot]) > 0)
            if rwidths[e] == 0:
                assert not flags & FLAG_REPLY_CHANGED, (t, e)
            if slot != int(choice.slot[e]):
                best = int(choice.slot[e])
                bound = _u_bound(behind[slot], behind[best], float(weights[e]))
                assert abs(float(u[best]) - float(u[slot])) <= bound, (t, e, u.tolist(), slot, best, bound)
                close_rows += 1
            elif bool(flags & FLAG_REPLY_CHANGED) != bool(choice.reply_changed[e]):
                # the kernel's one-ply choice is another one: only where the two one-ply u lie within the one-ply bound
                one = lookahead_choose(lf[e:e + 1, REC_CAND + W:REC_CAND + 2 * W].double(), torch.tensor([n]),
                                       rec["child_value_logits"][e:e + 1], rec["child_rewards"][e:e + 1],
                                       rec["child_done"][e:e + 1], float(weights[e]))
                top = np.sort(one.u[0, :n].numpy())[::-1]
                own = [[] if bool(rec["child_done"][e, j]) else [rec["child_value_logits"][e, j].numpy().astype(np.float64)]
                       for j in range(n)]
                assert n > 1 and top[0] - top[1] <= max(_u_bound(own[a], own[b], float(weights[e])) for a in range(n)
                                                        for b in range(n) if a != b), (t, e)
                close_rows += 1
            changed += int(bool(flags & FLAG_CHANGED))
            won += int(bool(flags & FLAG_WON))
            reply_changed += int(bool(flags & FLAG_REPLY_CHANGED))
            # a live chosen child is the env's next position, bit for bit
            if t + 1 < len(recs) and not bool(rec["child_done"][e, slot]):
                assert torch.equal(recs[t + 1]["obs"][e], rec["child_obs"][e * W + slot]), (t, e)
    print(f"active rows {active_rows} (of a reply_width 0 model {one_ply_rows}), rows within the fp32 bound that chose another "
          f"child {close_rows}, changed {changed}, differing from the one-ply choice {reply_changed}, children with replies "
          f"{backed_children}, finished grandchildren {done_grand}")
    s = stats.lookahead
    assert (active_rows, changed, won, reply_changed) == (s.searched, s.changed, s.won, s.reply_changed)
    assert active_rows > 100 and one_ply_rows > 20 and backed_children > 100 and reply_changed > 0
    assert close_rows <= 0.02 * active_rows


def _key(results):
    return [(r.a, r.b, r.a_wins, r.b_wins, r.draws, r.plies, r.partial) for r in results]


def _games(results):
    return [[(g.env, g.finished, tuple(int(a) for a in g.actions)) for g in r.recorded_games] for r in results]


def _arena(lookahead, graph, seed=23):
    return MatchArena(_group(), N, PER, MAX_PLY, sync_every=2, graph=graph, seed=seed, game_log=256, lookahead=lookahead)


def test_graph_equals_no_graph():
    eager, graph = _arena(CTL, False), _arena(CTL, True)
    r1, s1 = eager.run_round(PAIRINGS, games_per_match=4)
    r2, s2 = graph.run_round(PAIRINGS, games_per_match=4)
    assert graph._graph is not None and eager._graph is None
    assert _key(r1) == _key(r2) and s1.round_plies == s2.round_plies and _games(r1) == _games(r2)
    assert s1.lookahead == s2.lookahead and s1.lookahead.searched > 100 and s1.lookahead.reply_changed > 0
    assert torch.equal(eager.ply.stages["lookahead"].engine.records(), graph.ply.stages["lookahead"].engine.records())
    assert torch.equal(eager.ply.stages["lookahead"].engine.reply_records(), graph.ply.stages["lookahead"].engine.reply_records())
    assert torch.equal(eager.env.current().observations, graph.env.current().observations)


def test_reply_width_0_everywhere_plays_the_games_of_the_one_ply_arena():
    plain = _arena(ONE_PLY, True, seed=29)
    zero = _arena([LookaheadControls(3, 0.25, reply_width=0), LookaheadControls(2, 0.0, 4, 0)], True, seed=29)
    assert plain.ply.stages["lookahead"].engine._grand is None and zero.ply.stages["lookahead"].engine._grand is None and zero.ply.stages["lookahead"].engine.reply_width == 0    # nothing more is allocated
    assert np.array_equal(plain.ply.stages["lookahead"].table.cpu().numpy(), zero.ply.stages["lookahead"].table.cpu().numpy())
    r0, s0 = plain.run_round(PAIRINGS, games_per_match=4)
    r1, s1 = zero.run_round(PAIRINGS, games_per_match=4)
    assert _key(r0) == _key(r1) and _games(r0) == _games(r1) and s0.lookahead == s1.lookahead and s0.lookahead.reply_changed == 0
    # and an arena built for replies whose table says 0 everywhere: seven stages, the same games, move for move
    built = _arena(CTL, True, seed=29)
    built.set_lookahead(ONE_PLY)
    r2, s2 = built.run_round(PAIRINGS, games_per_match=4)
    assert _key(r0) == _key(r2) and _games(r0) == _games(r2) and s0.lookahead == s2.lookahead
    assert torch.equal(plain.ply.stages["lookahead"].engine.records(), built.ply.stages["lookahead"].engine.records())
    assert sum(len(g) for g in _games(r0)) >= 8


def test_set_lookahead_switches_the_replies_on_and_off_without_a_capture():
    arena, fresh = _arena(CTL, True, seed=31), _arena(CTL, True, seed=31)
    r0, s0 = arena.run_round(PAIRINGS, games_per_match=4)
    graph, table = arena._graph, arena.ply.stages["lookahead"].table
    assert graph is not None and s0.lookahead.reply_changed > 0
    arena.set_lookahead(ONE_PLY)
    assert table[:, 3].tolist() == [0, 0]
    r1, s1 = arena.run_round(PAIRINGS, games_per_match=4)
    assert s1.lookahead.reply_changed == 0 and s1.lookahead.searched > 100
    arena.set_lookahead(CTL)
    assert arena._graph is graph and arena.ply.stages["lookahead"].table is table and table[:, 3].tolist() == [2, 0]
    r2, s2 = arena.run_round(PAIRINGS, games_per_match=4)
    assert s2.lookahead.reply_changed > 0
    # the rounds depend on the table alone: a fresh arena plays the same three rounds
    f0, _ = fresh.run_round(PAIRINGS, games_per_match=4)
    assert _games(f0) == _games(r0)
    fresh.set_lookahead(ONE_PLY)
    f1, _ = fresh.run_round(PAIRINGS, games_per_match=4)
    fresh.set_lookahead(CTL)
    f2, t2 = fresh.run_round(PAIRINGS, games_per_match=4)
    assert _games(f1) == _games(r1) and _games(f2) == _games(r2) and t2.lookahead == s2.lookahead
    assert _games(r1) != _games(r0)


def test_refusals():
    with pytest.raises(ValueError, match="needs a width above 0"):
        LookaheadControls(0, reply_width=2)
    arena = MatchArena(_group(), N, PER, MAX_PLY, graph=False, lookahead=CTL)
    with pytest.raises(ValueError, match="above the reply_width"):
        arena.set_lookahead(LookaheadControls(3, reply_width=3))
    with pytest.raises(ValueError, match="above the width"):
        arena.set_lookahead(LookaheadControls(4, reply_width=2))
    arena.set_lookahead(LookaheadControls(3, reply_width=2))
    one = MatchArena(_group(), N, PER, MAX_PLY, graph=False, lookahead=ONE_PLY)
    with pytest.raises(ValueError, match="above the reply_width"):
        one.set_lookahead(CTL)
    env = VecEnv(4, 24, "katago", "spatial", output="torch", check_actions=True)
    env.reset()
    with pytest.raises(ValueError, match="reply_width must be an integer"):
        Lookahead(env, _group(), 3, 9)
    la = Lookahead(env, _group(), 3)
    for call in (lambda: la.fork_replies(None, 0), lambda: la.step_grandchildren(0), la.evaluate_grandchildren,
                 lambda: la.choose_replies(None, None, None, 0), la.reply_records):
        with pytest.raises(ValueError, match="reply_width=0"):
            call()
    with pytest.raises(_lib.KeiseiHipError, match="reply_width must lie in"):
        _lib.call("ka_lookahead_choose_replies", la._records, 3, la._records, 9, la._records, la.child_model_of, 1,
                  la.child_value_logits, la.child_rewards, la.child_terminated, la.child_truncated, None,
                  la.child_value_logits, la.child_rewards, la.child_terminated, la.child_truncated, None,
                  la.child_actions, la._counters, la._counters, 4, _stream())
