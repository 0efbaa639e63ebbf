"""The one-ply lookahead on the device: ka_lookahead_fork / ka_lookahead_choose against the float64 restatement, the forked
child rows against replayed games bit for bit, and MatchArena(lookahead=) ply by ply."""
import gc

import numpy as np
import pytest
import torch

from keisei_amd import _lib
from keisei_amd.shogi_gym import ACTION_SPACE, MASK_WORDS, VecEnv
from keisei_amd.training import (Lookahead, LookaheadControls, MatchArena, lookahead_active, lookahead_candidates,
                                 lookahead_choose, lookahead_table, sample_controlled)
from keisei_amd.training.lookahead import (FLAG_ACTIVE, FLAG_CHANGED, FLAG_WON, REC_ACTION, REC_CAND, REC_FLAGS, REC_NCAND,
                                           REC_SLOT)
from keisei_amd.training.model_group import SEResNetGroup
from keisei_amd.training.models.se_resnet import SEResNetModel, SEResNetParams
from oracle import keisei_oracle as orc
from oracle import shogi as S
from oracle.shogi import GOLD, KING, PAWN, WHITE, sq
from policy_insight_helpers import ATOL, RTOL

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPE = orc.NetShape(2, 128, 8, 64, 16, 128, 64)             # the smallest group the kernels accept: 128 channels, 2 blocks
OFF = LookaheadControls.OFF
_MODELS = []
_GROUP = {}


@pytest.fixture(autouse=True)
def _release_device_objects():
    """Arenas own captured graphs and pinned buffers: collect them with the device idle, not inside a later test's
    capture (tests/test_hip_league_rollout.py)."""
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


# ------------------------------------------------------------------ 1. candidates and priors
def _candidate_rows(width):
    """rows with 1, 3, width and width + 1 legal moves, ties across a word boundary of the mask, a crowded row; every
    logit is a bf16 value, so the fp32 and the bf16 tensors hold the same numbers"""
    rng = np.random.default_rng(100 + width)
    rows = [{4000: 0.5},
            {31: 1.0, 32: 1.0, 33: 0.25},                                   # tied across the boundary of words 0 and 1
            {int(a): float(v) for a, v in zip(rng.choice(ACTION_SPACE, width, replace=False), rng.integers(-8, 8, width) / 4)},
            {int(a): float(v) for a, v in zip(rng.choice(ACTION_SPACE, width + 1, replace=False),
                                              rng.integers(-8, 8, width + 1) / 4)},
            {63: -0.5, 64: -0.5, 95: -0.5, 96: -0.5, 11258: -0.5, 0: -0.75},  # every candidate tied, first and last action
            {int(a): float(v) for a, v in zip(rng.choice(ACTION_SPACE, 300, replace=False), rng.integers(-16, 16, 300) / 8)}]
    B = len(rows)
    logits = torch.full((B, ACTION_SPACE), 9.0)                             # illegal logits are the largest: they must not matter
    legal = torch.zeros(B, ACTION_SPACE, dtype=torch.bool)
    for b, d in enumerate(rows):
        for a, v in d.items():
            logits[b, a], legal[b, a] = v, True
    return logits, legal


@pytest.mark.parametrize("width", [1, 3, 8])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_candidates_and_priors_against_the_restatement(width, dtype):
    logits, legal = _candidate_rows(width)
    logits = logits.to(dtype)
    want_c, want_p, want_n = lookahead_candidates(logits, legal, width)
    assert want_n.tolist() == [1, min(3, width), width, width, min(6, width), width]
    for packed in (False, True):
        leg = legal.to(DEV)
        if packed:
            bits = torch.zeros(legal.shape[0], MASK_WORDS, dtype=torch.int32, device=DEV)
            _lib.call("ka_pack_mask_bits", leg.contiguous(), bits, legal.shape[0], ACTION_SPACE, _stream())
            leg = bits
        got_c, got_p, got_n = lookahead_candidates(logits.to(DEV), leg, width)
        assert torch.equal(got_c.cpu(), want_c) and torch.equal(got_n.cpu(), want_n)
        np.testing.assert_allclose(got_p.cpu().numpy().astype(np.float64), want_p.numpy(), rtol=RTOL, atol=ATOL)
    assert want_c[1].tolist()[:min(3, width)] == [31, 32, 33][:min(3, width)]
    assert want_c[4].tolist()[:min(6, width)] == [63, 64, 95, 96, 11258, 0][:min(6, width)]


def test_a_legal_inf_or_nan_logit_is_never_a_candidate_on_the_device():
    logits = torch.zeros(2, ACTION_SPACE)
    legal = torch.zeros(2, ACTION_SPACE, dtype=torch.bool)
    for a, v in {3: float("-inf"), 10: float("nan"), 64: 0.0, 65: -2.0}.items():
        logits[0, a], legal[0, a] = v, True
    logits[1, 7], legal[1, 7] = float("nan"), True
    want = lookahead_candidates(logits, legal, 4)
    got = lookahead_candidates(logits.to(DEV), legal.to(DEV), 4)
    assert got[0].cpu().tolist() == want[0].tolist() == [[64, 65, -1, -1], [-1, -1, -1, -1]]
    assert got[2].cpu().tolist() == [2, 0]
    np.testing.assert_allclose(got[1].cpu().numpy().astype(np.float64), want[1].numpy(), rtol=RTOL, atol=ATOL)


# ------------------------------------------------------------------ 2. fork fidelity
STEPS, WIDTH = 15, 3
MATE = S.encode(sq(1, 4), sq(1, 4), drop=GOLD)               # the gold drop on 5b


def _scripts():
    """Action histories of four envs, 15 plies each, checked move by move with the C oracle on the CPU; per env the move that
    is interesting at ply 15.
    (a) four pawn moves, then both golds step up and back: the position after ply 4 stands again after plies 8 and 12, and
        White's gold going home at ply 16 makes it the fourth time;
    (b) pawn pushes only: at max_ply = 16 it stands one ply under the ceiling;
    (c) via set_state, White to move: king 5a, against a pawn on 5c, a gold in hand and a king walking along the ninth rank;
        after 15 plies the gold drop on 5b mates;
    (d) a bishop exchange and seeded legal moves: an ordinary middlegame."""
    a = [S.encode(sq(6, 2), sq(5, 2)), S.encode(sq(2, 6), sq(3, 6), white=True), S.encode(sq(6, 7), sq(5, 7)),
         S.encode(sq(2, 1), sq(3, 1), white=True)]
    cycle = [S.encode(sq(8, 5), sq(7, 5)), S.encode(sq(0, 3), sq(1, 3), white=True), S.encode(sq(7, 5), sq(8, 5)),
             S.encode(sq(1, 3), sq(0, 3), white=True)]
    a = (a + cycle * 3)[:STEPS]
    b = [S.encode(sq(2, k // 2), sq(3, k // 2), white=True) if k % 2 else S.encode(sq(6, k // 2), sq(5, k // 2))
         for k in range(STEPS)]
    c = []
    for k in range(STEPS):
        if k % 2 == 0:
            f, t = (sq(0, 4), sq(0, 5)) if (k // 2) % 2 == 0 else (sq(0, 5), sq(0, 4))
            c.append(S.encode(f, t, white=True))
        else:
            c.append(S.encode(sq(8, k // 2), sq(8, k // 2 + 1)))
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
    for k in range(STEPS):
        if k >= len(d):
            d.append(int(rng.choice(np.flatnonzero(mask[3]))))
        acts = np.array([a[k], b[k], c[k], d[k]], dtype=np.int64)
        assert all(mask[i, acts[i]] for i in range(4)), (k, acts)
        r = ref.step(acts)
        assert not (r["terminated"] | r["truncated"]).any(), k
        mask = r["legal_masks"]
    # the facts the scenario rests on, by the oracle: the repetition, the mate
    r = ref.step(np.array([cycle[3], b[0], MATE, int(np.flatnonzero(mask[3])[0])], dtype=np.int64))
    assert r["terminated"][0] and r["termination_reason"][0] == S.R_REPETITION and r["rewards"][0] == 0.0
    assert r["terminated"][2] and r["termination_reason"][2] == S.R_CHECKMATE and r["rewards"][2] == 1.0
    return [a, b, c, d], (board, hands, 1), [cycle[3], None, MATE, None]


def _scenario(max_ply):
    """a device VecEnv of 4 envs after the scripts, crafted logits with the interesting move third, and the histories"""
    hist, start, special = _scripts()
    env = VecEnv(4, max_ply, "katago", "spatial", output="torch", check_actions=True)
    env.reset()
    env.set_state(2, *start)
    for k in range(STEPS):
        r = env.step(torch.tensor([h[k] for h in hist], dtype=torch.int64, device=DEV))
        assert not bool((r.terminated | r.truncated).any())
    masks = env.current().legal_masks.cpu().numpy()
    rng = np.random.default_rng(9)
    logits = torch.from_numpy(rng.uniform(-1.0, 0.0, (4, ACTION_SPACE)).astype(np.float32))
    for e in range(4):
        legal = np.flatnonzero(masks[e])
        third = special[e] if special[e] is not None else int(legal[len(legal) // 2])
        assert masks[e, third]
        others = [int(x) for x in legal if x != third][:2]
        logits[e, others[0]], logits[e, others[1]], logits[e, third] = 3.0, 2.5, 2.0
        special[e] = third
    return env, hist, start, logits.to(DEV), special


def _replay_children(hist, start, max_ply, cands):
    """a second VecEnv of 4 * width rows: row e * width + j replays env e's history from the same start, then plays
    candidate j"""
    rep = VecEnv(4 * WIDTH, max_ply, "katago", "spatial", output="torch", check_actions=True)
    rep.reset()
    for j in range(WIDTH):
        rep.set_state(2 * WIDTH + j, *start)
    for k in range(STEPS):
        rep.step(torch.tensor([h[k] for h in hist], dtype=torch.int64, device=DEV).repeat_interleave(WIDTH))
    return rep, rep.step(cands.reshape(-1).to(torch.int64))


@pytest.mark.parametrize("max_ply", [24, 23, 16])          # (history rows copied in 16-byte, 8-byte and single-byte pieces)
def test_forked_children_are_the_replayed_games_bit_for_bit(max_ply):
    """Four cases: (a) one move before a fourfold repetition, (b) one ply under max_ply, (c) a mate in one placed by
    set_state and (d) a middlegame, in one env of 4.  set_state restarts every game at ply 0, and an env steps all its games
    together, so every game of that env stands at the same ply -- and the env kernel lets the ply ceiling win over a
    repetition or a mate.  (a) and (c) can therefore not stand beside (b) in one env.  The same four scripts run under
    several ceilings instead: at max_ply = 24 and 23 the repetition and the mate happen in the children, at max_ply = 16
    every env, (b) among them, stands one ply under the ceiling and every child is truncated."""
    env, hist, start, logits, special = _scenario(max_ply)
    la = Lookahead(env, _group(), WIDTH)
    table = torch.from_numpy(lookahead_table(LookaheadControls(WIDTH), 1)).to(DEV)
    model_of = torch.zeros(4, dtype=torch.int32, device=DEV)
    cur = env.current()
    sampled = torch.tensor([int(np.flatnonzero(m)[0]) for m in cur.legal_masks.cpu().numpy()], dtype=torch.int64, device=DEV)
    before = [t.clone() for t in (env._state, env._keys, env._checks, cur.legal_mask_bits, cur.legal_masks, sampled)]
    la.fork(logits, cur.legal_mask_bits, sampled, model_of, table, _stream())
    la.step_children(_stream())
    torch.cuda.synchronize()
    after = (env._state, env._keys, env._checks, cur.legal_mask_bits, cur.legal_masks, sampled)
    assert all(torch.equal(x, y) for x, y in zip(before, after))           # the parent's rows are only read
    assert not bool(la._child_err.any())
    rec = la.records().cpu()
    cands = rec[:, REC_CAND:REC_CAND + WIDTH]
    assert rec[:, REC_NCAND].tolist() == [WIDTH] * 4 and rec[:, REC_FLAGS].tolist() == [FLAG_ACTIVE] * 4
    assert cands[:, 2].tolist() == special                                 # the interesting move is the third candidate
    want_c, want_p, _ = lookahead_candidates(logits.cpu(), cur.legal_masks.cpu(), WIDTH)
    assert torch.equal(cands, want_c)
    np.testing.assert_allclose(rec.view(torch.float32)[:, REC_CAND + WIDTH:REC_CAND + 2 * WIDTH].numpy().astype(np.float64),
                               want_p.numpy(), rtol=RTOL, atol=ATOL)
    assert torch.equal(la.child_actions.cpu(), cands.reshape(-1).to(torch.int64))
    assert la.child_model_of.cpu().tolist() == [0] * (4 * WIDTH)

    rep, r = _replay_children(hist, start, max_ply, cands.to(DEV))
    for name, got, want in (("observation", la.child_obs, r.observations), ("packed mask", la.child_mask_bits, r.legal_mask_bits),
                            ("reward", la.child_rewards, r.rewards), ("terminated", la.child_terminated, r.terminated),
                            ("truncated", la.child_truncated, r.truncated),
                            ("termination reason", la.child_reason, r.step_metadata.termination_reason),
                            ("current player", la.child_players, r.current_players)):
        assert got.dtype == want.dtype and torch.equal(got, want), name
    reason = la.child_reason.cpu().numpy().reshape(4, WIDTH)
    reward = la.child_rewards.cpu().numpy().reshape(4, WIDTH)
    if max_ply != 16:
        assert reason[0].tolist() == [S.R_PROGRESS, S.R_PROGRESS, S.R_REPETITION]          # needs the key history
        assert reason[1].tolist() == [S.R_PROGRESS] * 3 and reason[3].tolist() == [S.R_PROGRESS] * 3
        assert reason[2].tolist() == [S.R_PROGRESS, S.R_PROGRESS, S.R_CHECKMATE] and reward[2, 2] == 1.0
    else:
        assert (reason == S.R_MAXMOVES).all() and bool(la.child_truncated.all()) and not reward.any()


def test_unused_and_inactive_slots_get_the_sampled_action_and_no_model():
    env, hist, start, logits, special = _scenario(24)
    la = Lookahead(env, _group(), WIDTH)
    # env 0: width 3; env 1: off; env 2: skipped (its game ply 15 is below skip_plies); env 3: unseated
    table = torch.from_numpy(lookahead_table([LookaheadControls(3), OFF, LookaheadControls(3, skip_plies=16)], 3)).to(DEV)
    model_of = torch.tensor([0, 1, 2, -1], dtype=torch.int32, device=DEV)
    cur = env.current()
    masks = cur.legal_masks.cpu().numpy()
    sampled = torch.tensor([int(np.flatnonzero(m)[-1]) for m in masks], dtype=torch.int64, device=DEV)
    # env 0 has two usable logits only: its third slot is unused
    row = torch.full((ACTION_SPACE,), float("-inf"))
    legal0 = np.flatnonzero(masks[0])
    row[int(legal0[0])], row[int(legal0[1])] = 0.5, 1.5
    logits[0] = row.to(DEV)
    la.fork(logits, cur.legal_mask_bits, sampled, model_of, table, _stream())
    la.step_children(_stream())
    rec = la.records().cpu()
    assert rec[:, REC_FLAGS].tolist() == [FLAG_ACTIVE, 0, 0, 0] and rec[:, REC_NCAND].tolist() == [2, 0, 0, 0]
    assert rec[0, REC_CAND:REC_CAND + 3].tolist() == [int(legal0[1]), int(legal0[0]), -1]
    assert rec[1:, REC_CAND:REC_CAND + 3].eq(-1).all() and rec[:, REC_ACTION].tolist() == sampled.cpu().tolist()
    s = sampled.cpu().tolist()
    assert la.child_actions.cpu().tolist() == [int(legal0[1]), int(legal0[0]), s[0]] + [s[1]] * 3 + [s[2]] * 3 + [s[3]] * 3
    assert la.child_model_of.cpu().tolist() == [0, 0, -1] + [-1] * 9
    assert not bool(la._child_err.any())                                   # every child action was legal: nothing was held
    # choose leaves the inactive envs' actions alone
    la.evaluate()
    actions = sampled.clone()
    la.choose(actions, model_of, table, _stream())
    stats = la.read()
    assert actions[1:].cpu().tolist() == s[1:] and int(actions[0]) in (int(legal0[0]), int(legal0[1]))
    assert stats.searched == 1


# ------------------------------------------------------------------ 3. choose on synthetic inputs
def _synthetic(B, width, seed):
    """children whose u values differ by at least 1e-3 or not at all: q comes from five value-logit triples 0.3 apart (and
    the rewards -1, 0, 1), the priors are 0, 1/2 or 1 and the weight is 0.0371, so that equal (q, prior) pairs tie exactly and
    different ones lie at least 0.0371 / 2 apart"""
    rng = np.random.default_rng(seed)
    triples = np.array([[np.log((0.8 - q) / 2), np.log(0.2), np.log((0.8 + q) / 2)] for q in (-0.6, -0.3, 0.0, 0.3, 0.6)], np.float32)
    vl = torch.from_numpy(triples[rng.integers(0, 5, (B, width))])
    done = torch.from_numpy(rng.random((B, width)) < 0.2)
    rewards = torch.from_numpy(rng.integers(-1, 2, (B, width)).astype(np.float32)) * done
    priors = torch.from_numpy((rng.integers(0, 3, (B, width)) / 2).astype(np.float32))
    n_cand = torch.from_numpy(rng.integers(0, width + 1, B).astype(np.int32))
    n_cand[:4] = torch.tensor([0, 1, width, width])
    return priors, n_cand, vl, rewards, done


@pytest.mark.parametrize("width,weight", [(1, 0.0), (3, 0.0371), (8, 0.0), (8, 0.0371)])
def test_choose_against_the_restatement(width, weight):
    B = 300
    priors, n_cand, vl, rewards, done = _synthetic(B, width, 40 + width)
    want = lookahead_choose(priors, n_cand, vl, rewards, done, weight)
    u = np.sort(want.u.numpy(), axis=1)[:, ::-1]
    with np.errstate(invalid="ignore"):                                     # (-inf in the unused slots)
        gaps = u[:, :-1] - u[:, 1:] if width > 1 else np.zeros((B, 0))
    gaps = gaps[np.isfinite(gaps)]
    assert ((gaps == 0) | (gaps >= 1e-3)).all()                             # no row is ambiguous: none is left out
    assert (gaps == 0).sum() >= 10 or width == 1                            # and exact ties are among the rows
    got = lookahead_choose(priors.to(DEV), n_cand.to(DEV), vl.to(DEV), rewards.to(DEV), done.to(DEV), weight)
    assert got.error == 0 and want.error == 0
    assert torch.equal(got.slot.cpu(), want.slot) and int((want.slot < 0).sum()) >= 1
    used = (torch.arange(width)[None, :] < n_cand[:, None]).numpy()
    np.testing.assert_allclose(got.q.cpu().numpy()[used], want.q.numpy()[used], rtol=RTOL, atol=ATOL)


def test_inactive_rows_keep_their_action_and_the_flags_raise_from_read():
    env, hist, start, logits, special = _scenario(24)
    la = Lookahead(env, _group(), WIDTH)
    table = torch.from_numpy(lookahead_table([LookaheadControls(WIDTH), OFF], 2)).to(DEV)
    model_of = torch.tensor([0, 1, 0, 1], dtype=torch.int32, device=DEV)
    cur = env.current()
    sampled = torch.tensor([int(np.flatnonzero(m)[0]) for m in cur.legal_masks.cpu().numpy()], dtype=torch.int64, device=DEV)

    def run(poison=None):
        la.clear()
        actions = sampled.clone()
        la.fork(logits, cur.legal_mask_bits, actions, model_of, table, _stream())
        la.step_children(_stream())
        la.evaluate()
        if poison is not None:
            poison()
        la.choose(actions, model_of, table, _stream())
        return actions

    actions = run()
    stats = la.read()
    rec = la.records().cpu()
    assert stats.searched == 2 and rec[:, REC_FLAGS].bitwise_and(FLAG_ACTIVE).tolist() == [1, 0, 1, 0]
    assert actions[1].item() == sampled[1].item() and actions[3].item() == sampled[3].item()
    assert [int(actions[e]) for e in (0, 2)] == [int(rec[e, REC_CAND + int(rec[e, REC_SLOT])]) for e in (0, 2)]
    assert stats.changed == sum(int(actions[e] != sampled[e]) for e in (0, 2))
    assert [bool(rec[e, REC_FLAGS] & FLAG_CHANGED) for e in (0, 2)] == [bool(actions[e] != sampled[e]) for e in (0, 2)]

    def nan_in_a_live_child():                                # env 0, slot 0: a live child of an active env
        assert not bool(la.child_terminated[0] | la.child_truncated[0])
        la.child_value_logits[0, 1] = float("nan")
    run(nan_in_a_live_child)
    with pytest.raises(RuntimeError, match="non-finite value logits"):
        la.read()
    assert np.isneginf(la.records().cpu().view(torch.float32)[0, REC_CAND + 2 * WIDTH].item())

    def nan_in_a_finished_child():                            # env 2, slot 2 is the mate: its value logits are not looked at
        la.child_value_logits[2 * WIDTH + 2, 0] = float("inf")
    run(nan_in_a_finished_child)
    la.read()

    def refused_child_step():
        la._child_err[1] = (3 << 32) | 77
    actions = run(refused_child_step)
    assert torch.equal(actions, sampled)                      # nothing is chosen from children that did not move
    with pytest.raises(RuntimeError, match="child step refused"):
        la.read()
    la.clear()
    assert la.read().searched == 0


# ------------------------------------------------------------------ 7. the mate in one through Lookahead.step
def test_the_mate_in_one_is_chosen_from_third_place():
    env, hist, start, logits, special = _scenario(24)
    grp = _group()
    la = Lookahead(env, grp, WIDTH)
    table = torch.from_numpy(lookahead_table(LookaheadControls(WIDTH), 2)).to(DEV)
    model_of = torch.tensor([0, 1, 1, 0], dtype=torch.int32, device=DEV)
    cur = env.current()
    want_c, _, _ = lookahead_candidates(logits.cpu(), cur.legal_masks.cpu(), WIDTH)
    assert want_c[2].tolist()[2] == MATE                      # ranked third by the policy
    actions = want_c[:, 0].to(torch.int64).to(DEV)            # the sampler would have played the first
    la.clear()
    la.step(logits, cur.legal_mask_bits, actions, model_of, table, _stream())
    stats = la.read()
    rec = la.records().cpu()
    assert int(actions[2]) == MATE and rec[2, REC_SLOT] == 2 and rec[2, REC_ACTION] == MATE
    assert int(rec[2, REC_FLAGS]) == FLAG_ACTIVE | FLAG_CHANGED | FLAG_WON
    assert rec.view(torch.float32)[2, REC_CAND + 2 * WIDTH + 2].item() == 1.0
    assert stats.searched == 4 and stats.won == 1 and stats.changed >= 1
    assert not bool((rec[[0, 1, 3], REC_FLAGS] & FLAG_WON).any())
    # the repetition child of env 0 is a draw: q = 0 exactly
    assert rec.view(torch.float32)[0, REC_CAND + 2 * WIDTH + 2].item() == 0.0
    # and the move is legal: the env plays it and the game ends as a win for the mover
    r = env.step(actions)
    env.raise_if_refused()
    assert bool(r.terminated[2]) and float(r.rewards[2]) == 1.0


# ------------------------------------------------------------------ 4. - 6. the arena
N, PER, MAX_PLY = 8, 4, 20
PAIRINGS = [(0, 1), (1, 0), (1, 1)]                          # more pairings than slots, one model against itself
CTL = [LookaheadControls(3, 0.25), LookaheadControls(2, 0.0, skip_plies=4)]
U24 = 2.0 ** -24                                              # the unit roundoff of fp32


def _u_bound(vl_a, vl_b, weight):
    """How far apart two u values must lie in float64 for the fp32 kernel to be held to their order.  With u = 2^-24 the
    unit roundoff: a value logit minus the row maximum is exact up to u |x|, so expf sees an argument off by u |x| (a
    relative error u |x| of the result) and adds its own error, at most 2 ulp = 4u: each of e0, e1, e2 is off by at most
    r = (X + 4) u relatively, X the largest |logit - maximum| of the triple.  (e2 - e0) / (e0 + e1 + e2): the numerator is
    off by at most r (e0 + e2) + u |e2 - e0|, the sum by a relative r + 2u, the quotient adds u; with (e0 + e2) / sum <= 1
    and |q| <= 1 that is |dq| <= 2 r + 4u = (2 X + 12) u.  u_j = q + w p_j with the recorded fp32 prior: the product and the
    sum round once each, at most u (w + 1 + w).  Per child (2 X + 13 + 2 w) u; two children are compared, and a finished
    child's q (a reward of -1, 0 or 1) is exact, which only makes the bound generous."""
    def spread(vl):
        return float(np.max(np.max(vl) - vl)) if np.isfinite(vl).all() else 0.0
    return ((2 * spread(vl_a) + 13 + 2 * weight) + (2 * spread(vl_b) + 13 + 2 * weight)) * U24


def test_every_recorded_arena_ply_is_the_restatement():
    grp = _group()
    arena = MatchArena(grp, N, PER, MAX_PLY, sync_every=2, graph=False, seed=21, record=True, lookahead=CTL)
    results, stats = arena.run_round(PAIRINGS, games_per_match=4)
    recs = arena.record
    assert len(recs) >= 20 and stats.lookahead is not None and stats.lookahead.searched > 100
    table = lookahead_table(CTL, 2)
    W = 3
    active_rows = close_rows = changed = won = skipped = narrow = live_checked = 0
    for t, rec in enumerate(recs):
        mo = rec["model_of"]
        logits = grp.forward(rec["obs"].to(DEV), mo.to(DEV), check=False).policy_logits.reshape(N, ACTION_SPACE).cpu()
        widths, weights = lookahead_active(table, mo, rec["game_plies"], width=W)
        cand, prior, n_cand = lookahead_candidates(logits, rec["mask_bits"], W)
        lr = rec["lookahead_records"]
        lf = lr.view(torch.float32)
        choice = None
        # what the sampler drew before the lookahead: the play sampler is the neutral row of the sampling controls
        sampled = sample_controlled(logits.to(DEV), rec["mask_bits"].to(DEV), rec["seed"], controls=None, model_of=mo.to(DEV),
                                    num_models=2).actions.cpu()
        for e in range(N):
            w = int(widths[e])
            n = min(w, int(n_cand[e]))
            flags = int(lr[e, REC_FLAGS])
            assert bool(flags & FLAG_ACTIVE) == (n > 0), (t, e)
            assert int(lr[e, REC_ACTION]) == int(rec["actions"][e]), (t, e)    # the stepped action is the recorded choice
            if n == 0:
                skipped += int(mo[e] == 1 and int(rec["game_plies"][e]) < 4)
                assert flags == 0 and int(lr[e, REC_NCAND]) == 0 and lr[e, REC_CAND:REC_CAND + W].eq(-1).all(), (t, e)
                assert int(rec["actions"][e]) == int(sampled[e]), (t, e)       # an inactive env keeps the sampler's action
                continue
            active_rows += 1
            narrow += int(w < W)
            # the candidates are the restatement's on the recomputed logits
            assert int(lr[e, REC_NCAND]) == n, (t, e)
            assert lr[e, REC_CAND:REC_CAND + W].tolist() == cand[e, :n].tolist() + [-1] * (W - n), (t, e)
            np.testing.assert_allclose(lf[e, REC_CAND + W:REC_CAND + W + n].numpy().astype(np.float64), prior[e, :n].numpy(),
                                       rtol=RTOL, atol=ATOL)
            # the choice is the restatement's on the recorded child outputs
            if choice is None:
                choice = lookahead_choose(lf[:, REC_CAND + W:REC_CAND + 2 * W].double(),
                                          torch.from_numpy(np.minimum(widths, n_cand.numpy())), rec["child_value_logits"],
                                          rec["child_rewards"], rec["child_done"], torch.from_numpy(weights))
                assert choice.error == 0
            slot = int(lr[e, REC_SLOT])
            u = choice.u[e, :n].numpy()
            np.testing.assert_allclose(lf[e, REC_CAND + 2 * W:REC_CAND + 2 * W + n].numpy().astype(np.float64),
                                       choice.q[e, :n].numpy(), rtol=RTOL, atol=ATOL)
            assert 0 <= slot < n and int(lr[e, REC_ACTION]) == int(lr[e, REC_CAND + slot]), (t, e)
            assert bool(flags & FLAG_CHANGED) == (int(lr[e, REC_ACTION]) != int(sampled[e])), (t, e)
            assert bool(flags & FLAG_WON) == (bool(rec["child_done"][e, slot]) and float(rec["child_rewards"][e, slot]) > 0)
            won += int(bool(flags & FLAG_WON))
            if slot != int(choice.slot[e]):
                best = int(choice.slot[e])
                bound = _u_bound(rec["child_value_logits"][e, slot].numpy().astype(np.float64),
                                 rec["child_value_logits"][e, best].numpy().astype(np.float64), float(weights[e]))
                assert abs(float(u[best]) - float(u[slot])) <= bound, (t, e, u.tolist(), slot, best, bound)
                close_rows += 1
            changed += int(bool(flags & FLAG_CHANGED))
            # a live chosen child is the env's next position, bit for bit
            c = e * W + slot
            if t + 1 < len(recs) and not bool(rec["child_done"][e, slot]):
                assert not bool(rec["terminated"][e] | rec["truncated"][e]), (t, e)
                assert torch.equal(recs[t + 1]["obs"][e], rec["child_obs"][c]), (t, e)
                assert torch.equal(recs[t + 1]["mask_bits"][e], rec["child_mask_bits"][c]), (t, e)
                live_checked += 1
            elif bool(rec["child_done"][e, slot]):
                assert bool(rec["terminated"][e] | rec["truncated"][e]), (t, e)
                assert float(rec["rewards"][e]) == float(rec["child_rewards"][e, slot]), (t, e)
    print(f"active rows {active_rows}, rows within the fp32 bound that chose the other child {close_rows}, "
          f"changed {changed}, skipped openings {skipped}, width-2 rows {narrow}, live children checked {live_checked}")
    assert (active_rows, changed, won) == (stats.lookahead.searched, stats.lookahead.changed, stats.lookahead.won)
    assert active_rows > 100 and narrow > 20 and skipped > 4 and live_checked > 100
    assert close_rows <= 0.02 * active_rows


def _key(results):
    return [(r.a, r.b, r.a_wins, r.b_wins, r.draws, r.plies, r.partial) for r in results]


def _games(results):
    return [[(g.env, g.finished, tuple(int(a) for a in g.actions)) for g in r.recorded_games] for r in results]


def test_graph_equals_no_graph():
    eager = MatchArena(_group(), N, PER, MAX_PLY, sync_every=2, graph=False, seed=23, game_log=256, lookahead=CTL)
    graph = MatchArena(_group(), N, PER, MAX_PLY, sync_every=2, graph=True, seed=23, game_log=256, lookahead=CTL)
    r1, s1 = eager.run_round(PAIRINGS, games_per_match=4)
    r2, s2 = graph.run_round(PAIRINGS, games_per_match=4)
    assert graph._graph is not None and eager._graph is None
    assert _key(r1) == _key(r2) and s1.round_plies == s2.round_plies and _games(r1) == _games(r2)
    assert s1.lookahead == s2.lookahead and s1.lookahead.searched > 100 and s1.lookahead.changed > 0
    assert torch.equal(eager.ply.stages["lookahead"].engine.records(), graph.ply.stages["lookahead"].engine.records())
    assert torch.equal(eager.env.current().observations, graph.env.current().observations)


def test_rows_that_are_off_play_the_games_of_no_lookahead_and_set_lookahead_needs_no_capture():
    plain = MatchArena(_group(), N, PER, MAX_PLY, sync_every=2, graph=True, seed=29, game_log=256)
    arena = MatchArena(_group(), N, PER, MAX_PLY, sync_every=2, graph=True, seed=29, game_log=256, lookahead=CTL)
    assert "lookahead" not in plain.ply.stages and arena.ply.stages["lookahead"].engine.width == 3
    arena.set_lookahead(OFF)                                  # the launches stay in the ply, every row is off
    r0, s0 = plain.run_round(PAIRINGS, games_per_match=4)
    r1, s1 = arena.run_round(PAIRINGS, games_per_match=4)
    assert s0.lookahead is None and s1.lookahead.searched == 0 and s1.lookahead.changed == 0
    assert _key(r0) == _key(r1) and _games(r0) == _games(r1) and sum(len(g) for g in _games(r0)) >= 8
    graph, table = arena._graph, arena.ply.stages["lookahead"].table
    assert graph is not None
    arena.set_lookahead(CTL)
    r2, s2 = arena.run_round(PAIRINGS, games_per_match=4)
    assert arena._graph is graph and arena.ply.stages["lookahead"].table is table
    assert s2.lookahead.searched > 100 and s2.lookahead.changed > 0 and _games(r2) != _games(r0)
    arena.set_lookahead(None)
    assert not bool(table.any())
    arena.set_lookahead([OFF, LookaheadControls(1)])
    assert np.array_equal(table.cpu().numpy(), lookahead_table([OFF, LookaheadControls(1)], 2))
    # an arena whose rows are all off at construction allocates nothing and launches nothing
    idle = MatchArena(_group(), N, PER, MAX_PLY, sync_every=2, graph=True, seed=29, game_log=256, lookahead=OFF)
    assert idle.ply.stages["lookahead"].engine is None and idle.ply.stages["lookahead"].table is not None
    r3, s3 = idle.run_round(PAIRINGS, games_per_match=4)
    assert _key(r3) == _key(r0) and _games(r3) == _games(r0) and s3.lookahead.searched == 0
    with pytest.raises(ValueError, match="above the width"):
        idle.set_lookahead(LookaheadControls(1))


def test_refusals():
    with pytest.raises(ValueError, match="collect=True"):
        MatchArena(_group(), N, PER, MAX_PLY, collect=True, lookahead=CTL)
    arena = MatchArena(_group(), N, PER, MAX_PLY, graph=False, lookahead=CTL)
    with pytest.raises(ValueError, match="above the width"):
        arena.set_lookahead(LookaheadControls(4))
    with pytest.raises(ValueError, match="expected 2"):
        arena.set_lookahead([OFF])
    plain = MatchArena(_group(), N, PER, MAX_PLY, graph=False)
    with pytest.raises(ValueError, match="built without lookahead"):
        plain.set_lookahead(OFF)
