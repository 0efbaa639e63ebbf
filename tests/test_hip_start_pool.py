"""Games started from a device-resident pool of positions (ka_shogi_env_reset_pool / ka_shogi_env_step_pool): the env against
the C oracle bit for bit with the restarts placed by the host restatement of the draw, clearing the pool, the validation
of an upload, the three device epochs over a pooled env, and a pool taken from game records.

One wave owns one game, so the shapes are tiny: what is at stake is the restart path (reset, checkmate, move limit), the
perspective flip of a white-to-move start and the game counter."""
import gc

import numpy as np
import pytest
import torch

from keisei_amd.shogi_gym import ACTION_SPACE, VecEnv, parse_sfen, start_pool_index
from keisei_amd.sl import prepare as prep
from keisei_amd.sl.parsers import GameFilter, SFENParser, is_standard_start
from keisei_amd.training import LeagueRollout, MatchArena, SelfPlayRollout
from keisei_amd.training.katago_ppo import KataGoRolloutBuffer
from keisei_amd.training.model_group import SEResNetGroup
from keisei_amd.training.models.se_resnet import SEResNetModel, SEResNetParams
from oracle import keisei_oracle as orc
from oracle import shogi as S
from sl_prepare_helpers import FILES
from start_pool_helpers import (IN_CHECK, MATE_INDEX, START, PooledOracle, choose_actions, mate_in_one, pool7,
                                pool_observation)

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPE = orc.NetShape(2, 128, 8, 64, 16, 128, 64)                 # the shape tests/test_hip_selfplay_rollout.py uses
OBS = (50, 9, 9)
SEED = 7              # with it the K = 7 run below restarts 30 times, by checkmate and by the move limit, and draws every row
STEP_KEYS = ("observations", "legal_masks", "rewards", "terminated", "truncated", "terminal_observations", "current_players")
META_KEYS = ("captured_piece", "termination_reason", "ply_count", "material_balance")
_MODELS = {}


@pytest.fixture(autouse=True)
def _release_device_objects():
    """(see tests/test_hip_selfplay_rollout.py: rollout objects own captured graphs and pinned buffers)"""
    yield
    gc.collect()
    torch.cuda.synchronize()
    gc.collect()


def _model(salt):
    if salt not in _MODELS:
        m = SEResNetModel(SEResNetParams(**SHAPE.__dict__))
        m.load_state_dict(orc.init_like_state_dict(SHAPE, salt=salt), strict=True)
        _MODELS[salt] = m.to(DEV).eval()
    return _MODELS[salt]


def _pack(mask: np.ndarray) -> np.ndarray:
    """bool rows -> the packed rows of the device rollout store (bit j of word w = action 32 w + j)"""
    n, A = mask.shape
    words = (A + 31) // 32
    padded = np.zeros((n, words * 32), np.uint64)
    padded[:, :A] = mask
    return (padded.reshape(n, words, 32) << np.arange(32, dtype=np.uint64)).sum(axis=2).astype(np.uint32)


def _bits(env: VecEnv) -> np.ndarray:
    return env._bits[env._cur].cpu().numpy().view(np.uint32)


def _games(env: VecEnv) -> np.ndarray:
    return env._state[:, 116:120].cpu().numpy().copy().view(np.uint32).reshape(-1)


def _subset(pool, rows):
    rows = list(rows)
    return tuple(x[rows] for x in pool)


# ------------------------------------------------------------------ 1. against the C oracle
def _oracle_run(K, n=5, max_ply=12, steps=60):
    """The oracle side alone: (pool, per-step actions and results, restarts, reasons, rows drawn)."""
    pool = pool7() if K == 7 else _subset(pool7(), [MATE_INDEX])
    mate_index, mate_action = (MATE_INDEX if K == 7 else 0), mate_in_one()[3]
    po = PooledOracle(n, max_ply, pool, SEED)
    first = po.reset()
    rng = np.random.default_rng(0)
    mask, trace, reasons = first[1], [], []
    for _ in range(steps):
        acts = choose_actions(po, mask, rng, mate_index, mate_action)
        r = po.step(acts)
        done = r["terminated"] | r["truncated"]
        reasons += r["termination_reason"][done].tolist()
        trace.append((acts, r, po.ref.stats(), po.games.copy()))
        mask = r["legal_masks"]
    return pool, po, first, trace, reasons


@pytest.mark.parametrize("K", [7, 1])
def test_pooled_env_equals_the_oracle_bit_for_bit(K):
    """K = 7: the whole pool; SEED makes the run restart 30 times, by checkmate and by the move limit, and draw every row.
    K = 1: the mate in one alone, the mating move played whenever it is offered -- every env restarts at every step (300
    restarts, all by checkmate; the move-limit restart belongs to the K = 7 run)."""
    pool, po, first, trace, reasons = _oracle_run(K)
    # conditions on the inputs (they hold on the oracle side alone)
    assert len(reasons) >= 30, len(reasons)
    assert S.R_CHECKMATE in reasons
    if K == 7:
        assert S.R_MAXMOVES in reasons and set(po.drawn) == set(range(7)), (set(reasons), set(po.drawn))
    dev = VecEnv(5, 12, "katago", "spatial", start_pool_capacity=8)
    assert dev.start_pool_count == 0
    dev.set_start_positions(*pool, seed=SEED)
    assert dev.start_pool_count == K and dev.start_pool_capacity == 8
    r0 = dev.reset()
    assert np.array_equal(r0.observations, first[0]) and np.array_equal(r0.legal_masks, first[1])
    assert np.array_equal(dev._players[0].cpu().numpy(), first[2]) and np.array_equal(_bits(dev), _pack(first[1]))
    assert not _games(dev).any()
    for t, (acts, rr, stats, games) in enumerate(trace):
        rd = dev.step(acts)
        for k in STEP_KEYS:
            assert np.array_equal(getattr(rd, k), rr[k]), (t, k)
        for k in META_KEYS:
            assert np.array_equal(getattr(rd.step_metadata, k), rr[k]), (t, k)
        assert np.array_equal(_bits(dev), _pack(rr["legal_masks"])), t
        assert np.array_equal(_games(dev), games), t
        assert (dev.episodes_completed, dev.episodes_drawn, dev.episodes_truncated, dev._stat(3)) == \
            (stats["episodes_completed"], stats["episodes_drawn"], stats["episodes_truncated"], stats["total_episode_ply"]), t
    assert dev.episodes_completed == len(reasons)
    # reset() draws game 0 again
    r0 = dev.reset()
    assert np.array_equal(r0.observations, first[0]) and np.array_equal(r0.legal_masks, first[1])
    assert np.array_equal(dev._players[0].cpu().numpy(), first[2]) and not _games(dev).any()
    want = start_pool_index(SEED, np.arange(5), 0, K)
    for e in range(5):
        board, hands, side, ply = dev.get_state(e)
        assert np.array_equal(board, pool[0][want[e]]) and np.array_equal(hands, pool[1][want[e]])
        assert side == pool[2][want[e]] and ply == 0


# ------------------------------------------------------------------ 2. clearing the pool
def _same_envs(envs, steps, seed):
    """Drive the envs with the same seeded random legal actions; every output and the positions must agree."""
    res = [e.reset() for e in envs]
    for r in res[1:]:
        assert np.array_equal(r.observations, res[0].observations) and np.array_equal(r.legal_masks, res[0].legal_masks)
    rng = np.random.default_rng(seed)
    mask = res[0].legal_masks
    for t in range(steps):
        acts = np.array([rng.choice(np.flatnonzero(m)) for m in mask], dtype=np.int64)
        res = [e.step(acts) for e in envs]
        for r, e in zip(res[1:], envs[1:]):
            for k in STEP_KEYS:
                assert np.array_equal(getattr(r, k), getattr(res[0], k)), (t, k)
            for k in META_KEYS:
                assert np.array_equal(getattr(r.step_metadata, k), getattr(res[0].step_metadata, k)), (t, k)
            assert np.array_equal(_bits(e), _bits(envs[0])), t
            assert torch.equal(e._state[:, :116], envs[0]._state[:, :116]), t
            assert torch.equal(e._stats, envs[0]._stats), t
        mask = res[0].legal_masks
    return envs[0].episodes_completed


def test_a_cleared_and_a_never_filled_pool_are_the_standard_start():
    plain = VecEnv(8, 30, "katago", "spatial")
    cleared = VecEnv(8, 30, "katago", "spatial", start_pool_capacity=8)
    empty = VecEnv(8, 30, "katago", "spatial", start_pool_capacity=8)
    cleared.set_start_positions(*pool7(), seed=3)
    r = cleared.reset()
    assert not np.array_equal(r.observations, plain.reset().observations)       # the pool was in use
    for _ in range(3):
        cleared.step(np.array([np.flatnonzero(m)[0] for m in cleared.current().legal_masks], dtype=np.int64))
    cleared.clear_start_positions()
    assert cleared.start_pool_count == 0
    cleared.reset_stats()
    finished = _same_envs([plain, cleared, empty], 40, 1)
    assert finished >= 8                                                        # restarts happened (max_ply 30 < 40 steps)
    assert not plain._state[:, 116:120].any()                                   # the kernel without a pool keeps no count


# ------------------------------------------------------------------ 3. validation
def _start():
    return parse_sfen(START)


def _edit(sfen, edits=(), hand=None):
    b, h, s = parse_sfen(sfen)
    for sq, pc in edits:
        b[sq] = pc
    if hand is not None:
        h[hand[0], hand[1]] += 1
    return b, h, s


BAD_POSITIONS = {
    "piece-byte": (_edit(START, [(40, 9)]), "board byte is no piece"),
    "missing-king": (_edit(START, [(76, 0)]), "black needs exactly one king"),
    "two-kings": (_edit(START, [(40, S.KING | S.WHITE)]), "white needs exactly one king"),
    "set-exceeded": (_edit(START, hand=(1, 5)), "more than 2 B"),
    "pawn-last-rank": (parse_sfen("P3k4/9/9/9/9/9/9/9/4K4 b - 1"), "pawn or lance stands on its last rank"),
    "lance-last-rank": (parse_sfen("4k4/9/9/9/9/9/9/9/4K3l b - 1"), "pawn or lance stands on its last rank"),
    "knight-last-two": (parse_sfen("4k4/N8/9/9/9/9/9/9/4K4 b - 1"), "knight stands on its last two ranks"),
    "two-pawns-on-a-file": (_edit(START, [(5 * 9, S.PAWN), (6 * 9 + 1, 0)]), "two unpromoted pawns of one colour on a file"),
    "other-side-in-check": (parse_sfen(IN_CHECK.replace(" b ", " w ")), "side not to move is in check"),
    "no-legal-move": (parse_sfen("4k4/4G4/4P4/9/9/9/9/9/4K4 w - 1"), "side to move has no legal move"),
}


@pytest.fixture(scope="module")
def busy_env():
    """An env with a pool in use and games in progress."""
    env = VecEnv(4, 30, "katago", "spatial", start_pool_capacity=4)
    env.set_start_positions(*_subset(pool7(), [1, 4, 6]), seed=2)
    env.reset()
    for _ in range(3):
        env.step(np.array([np.flatnonzero(m)[0] for m in env.current().legal_masks], dtype=np.int64))
    return env


def _snapshot(env):
    return [t.clone() for t in (env._state, env._pool, env._pool_hdr, env._obs[env._cur], env._mask[env._cur],
                                env._bits[env._cur], env._keys, env._checks, env._stats)]


@pytest.mark.parametrize("at", [0, 2])
@pytest.mark.parametrize("case", list(BAD_POSITIONS))
def test_a_refused_upload_names_the_index_and_changes_nothing(busy_env, case, at):
    (board, hands, side), text = BAD_POSITIONS[case]
    rows = [_start(), _start(), _start()]
    rows[at] = (board, hands, side)
    before = _snapshot(busy_env)
    with pytest.raises(ValueError, match=f"start position {at} is not playable: .*{text}"):
        busy_env.set_start_positions(np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]),
                                     np.array([r[2] for r in rows], np.uint8), seed=99)
    assert all(torch.equal(a, b) for a, b in zip(before, _snapshot(busy_env)))
    assert busy_env.start_pool_count == 3


def test_the_first_bad_index_wins_and_too_many_positions_are_refused(busy_env):
    bad_static, bad_dynamic = BAD_POSITIONS["piece-byte"][0], BAD_POSITIONS["no-legal-move"][0]
    before = _snapshot(busy_env)
    for rows, at, text in (([_start(), bad_dynamic, bad_static], 1, "no legal move"),
                           ([_start(), bad_static, bad_dynamic], 1, "no piece")):
        with pytest.raises(ValueError, match=f"start position {at} is not playable: .*{text}"):
            busy_env.set_start_positions(np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows]),
                                         np.array([r[2] for r in rows], np.uint8))
    five = [_start()] * 5
    with pytest.raises(ValueError, match="5 start positions do not fit start_pool_capacity=4"):
        busy_env.set_start_positions(np.stack([r[0] for r in five]), np.stack([r[1] for r in five]), np.zeros(5, np.uint8))
    with pytest.raises(ValueError, match="invalid SFEN"):
        busy_env.set_start_sfens([START, START.replace(" b ", " x ")])
    assert all(torch.equal(a, b) for a, b in zip(before, _snapshot(busy_env)))
    with pytest.raises(ValueError, match="no start pool"):
        VecEnv(2, 30, "katago", "spatial").set_start_positions(_start()[0][None], _start()[1][None], np.zeros(1, np.uint8))
    # tensors and the (K, 14) form are taken; SFEN strings too
    busy_env.set_start_positions(torch.from_numpy(_start()[0][None]), torch.from_numpy(_start()[1].reshape(1, 14)),
                                 torch.zeros(1, dtype=torch.uint8), seed=1)
    assert busy_env.start_pool_count == 1
    busy_env.set_start_sfens([START, IN_CHECK], seed=5)
    assert busy_env.start_pool_count == 2
    assert busy_env._pool_hdr.cpu().tolist() == [2, 0, 5, 0]


# ------------------------------------------------------------------ 4. SelfPlayRollout
POOL4 = [1, 2, 3, 6]           # white to move, in check, handicap (white to move), ply 30 of a game
POOL3 = [0, 4, 5]
ROLL_SEED, ROLL_SEED2 = 9, 11
COLUMNS = ("observations", "actions", "log_probs", "values", "rewards", "dones", "terminated", "legal_masks",
           "value_categories", "score_targets", "next_value_override")


def _pool_obs(rows, max_ply):
    pool = _subset(pool7(), rows)
    return pool, [torch.from_numpy(pool_observation(pool, i, max_ply)[0]) for i in range(len(rows))]


def _bitwise(a: torch.Tensor, b: torch.Tensor) -> bool:
    if a.dtype.is_floating_point:
        return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


def _selfplay(graph, sync_every):
    roll = SelfPlayRollout(_model(7), num_envs=8, max_ply=6, sync_every=sync_every, graph=graph, seed=4242,
                           start_pool_capacity=4)
    roll.env.set_start_positions(*_subset(pool7(), POOL4), seed=ROLL_SEED)
    roll.reset()
    buf = KataGoRolloutBuffer(8, OBS, ACTION_SPACE, device=DEV)
    roll.collect(buf, 24)
    return roll, {k: v.clone() for k, v in buf.flatten().items()}


def _check_starts(cols, games, seed, rows, first_row_is_a_start):
    """Every row behind a done row of env e shows the pool row the draw names; `games` counts on across calls."""
    _, want = _pool_obs(rows, 6)
    obs = cols["observations"].view(24, 8, *OBS).cpu()
    done = cols["dones"].view(24, 8).bool().cpu().numpy()
    checked = 0
    for e in range(8):
        if first_row_is_a_start:
            assert torch.equal(obs[0, e], want[int(start_pool_index(seed, e, 0, len(rows)))]), e
        for t in range(24):
            if done[t, e]:
                games[e] += 1
                if t + 1 < 24:
                    assert torch.equal(obs[t + 1, e], want[int(start_pool_index(seed, e, int(games[e]), len(rows)))]), (t, e)
                    checked += 1
    return checked


def test_selfplay_rollout_over_a_pool_with_and_without_a_graph():
    roll, graphed = _selfplay(True, 4)
    _, eager = _selfplay(False, 1)
    for k in COLUMNS:
        assert _bitwise(graphed[k], eager[k]), k
    games = np.zeros(8, np.int64)
    assert _check_starts(graphed, games, ROLL_SEED, POOL4, True) >= 3 * 8          # max_ply 6: a restart every six plies
    sides = _subset(pool7(), POOL4)[2]
    first = start_pool_index(ROLL_SEED, np.arange(8), 0, 4)
    assert sides[first].any()                                                     # a game that white opens
    assert np.array_equal(_games(roll.env).astype(np.int64), games)
    # another pool, on the captured graph: no reset, no capture
    graphs = dict(roll._graphs)
    roll.env.set_start_positions(*_subset(pool7(), POOL3), seed=ROLL_SEED2)
    buf = KataGoRolloutBuffer(8, OBS, ACTION_SPACE, device=DEV)
    roll.collect(buf, 24)
    assert roll._graphs == graphs and graphs
    assert _check_starts(buf.flatten(), games, ROLL_SEED2, POOL3, False) >= 3 * 8
    assert np.array_equal(_games(roll.env).astype(np.int64), games)


# ------------------------------------------------------------------ 5. MatchArena and LeagueRollout
PLY_PLANE, BLACK_PLANE = 28 + 15, 28 + 14


def _arena_round(rows, seed):
    group = SEResNetGroup([_model(5), _model(34)])
    arena = MatchArena(group, 8, 4, 6, sync_every=4, graph=True, seed=11, collect=True, start_pool_capacity=4)
    arena.env.set_start_positions(*_subset(pool7(), rows), seed=seed)
    results, stats = arena.run_round([(0, 1), (1, 0)], games_per_match=6, trainable={0: 3, 1: 3})
    arena.env.raise_if_refused()
    return arena, results, stats


@pytest.mark.parametrize("rows", [POOL4, [1, 3]], ids=["mixed", "white-to-move-only"])
def test_match_arena_plays_from_the_pool(rows):
    arena, results, stats = _arena_round(rows, 5)
    _, want = _pool_obs(rows, 6)
    sides = _subset(pool7(), rows)[2]
    assert len(results) == 2 and stats.total_games == sum(r.a_wins + r.b_wins + r.draws for r in results)
    for r in results:
        assert not r.partial and r.a_wins + r.b_wins + r.draws == r.games >= 6
        ro = r.rollout
        assert ro is not None
        obs = ro.observations.view(-1, *OBS).cpu()
        starts = (obs[:, PLY_PLANE, 0, 0] == 0).nonzero().reshape(-1).tolist()      # ply 0: a game's first position
        assert len(starts) > 4                                                      # more than the four opening games
        for i in starts:
            hit = [j for j, w in enumerate(want) if torch.equal(obs[i], w)]
            assert hit, i
            assert int(ro.perspective[i]) == int(sides[hit[0]])
            assert float(obs[i, BLACK_PLANE, 0, 0]) == float(sides[hit[0]] == 0)
        assert float(ro.dones.sum()) > 0


def test_league_rollout_plays_from_the_pool():
    roll = LeagueRollout(_model(5), [_model(34)], [1], num_envs=8, max_ply=6, sync_every=4, graph=True, seed=3,
                         start_pool_capacity=4)
    roll.env.set_start_positions(*_subset(pool7(), POOL4), seed=ROLL_SEED)
    roll.reset()
    before = roll.env.episodes_completed
    buf = KataGoRolloutBuffer(8, OBS, ACTION_SPACE, device=DEV)
    stats = roll.collect(buf, 24)
    roll.env.raise_if_refused()                                                   # no latched refusal
    assert stats.plies == 24 and stats.rows > 0
    assert stats.wins + stats.losses + stats.draws == stats.terminated
    assert stats.terminated + stats.truncated == roll.env.episodes_completed - before >= 3 * 8
    assert int(_games(roll.env).sum()) == stats.terminated + stats.truncated       # every finished game drew its successor


# ------------------------------------------------------------------ 6. a pool from game records
def _opening_host(path, ply, min_ply):
    """The same records through the oracle env on the host: the first 96 state bytes of every game still legal and
    unfinished after `ply` moves, duplicates dropped, first seen first."""
    seen, rows = set(), []
    for rec in SFENParser().parse(path):
        if not GameFilter(min_ply=min_ply).accepts(rec) or not is_standard_start(rec.start):
            continue
        actions, _ = prep._encode_game(rec, ply)
        if len(actions) < ply:
            continue
        env = S.OracleVecEnv(1, ply + 1)
        _, mask = env.reset()
        ok = True
        for a in actions:
            if not mask[0, a]:
                ok = False
                break
            r = env.step(np.array([a], np.int64))
            if r["terminated"][0] or r["truncated"][0]:
                ok = False
                break
            mask = r["legal_masks"]
        if not ok:
            continue
        board, hands, side, _ = env.state(0)
        row = np.concatenate([board, hands.reshape(14), [side]]).astype(np.uint8)
        if row.tobytes() not in seen:
            seen.add(row.tobytes())
            rows.append(row)
    return np.stack(rows)


def test_opening_positions_equal_the_oracle_replay():
    boards, hands, sides = prep.opening_positions([str(FILES[0])], 8, min_ply=1, batch_envs=4)
    want = _opening_host(FILES[0], 8, 1)
    got = np.concatenate([boards, hands.reshape(-1, 14), sides[:, None]], axis=1)
    assert got.dtype == np.uint8 and got.shape == want.shape and len(want) >= 4
    assert {r.tobytes() for r in got} == {r.tobytes() for r in want} and len({r.tobytes() for r in got}) == len(got)
    assert np.array_equal(got, want)                                              # and in first-seen order
    assert not sides.any()                                                        # black is to move after eight plies
    capped = prep.opening_positions([str(FILES[0])], 8, min_ply=1, batch_envs=4, max_positions=3)
    assert np.array_equal(capped[0], boards[:3])
    env = VecEnv(4, 30, "katago", "spatial", start_pool_capacity=len(got))
    env.set_start_positions(boards, hands, sides, seed=1)
    assert env.start_pool_count == len(got)
    first = start_pool_index(1, np.arange(4), 0, len(got))
    env.reset()
    for e in range(4):
        assert np.array_equal(env.get_state(e)[0], boards[first[e]])
