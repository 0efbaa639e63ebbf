"""The spectator feed on the device: `VecEnv.get_spectator_data()` and the move notes of csrc/spectator.hip
(ka_spectator_note / ka_spectator_commit / ka_spectator_begin) against the host restatement `host_move_note`, word for word,
in lockstep with the CPU oracle; clearing at the end of a game, refused steps, guard bands around every buffer the kernels
touch, and the histories inside captured plies against the game log, a mechanism they share no code with.

One wave owns one env, so the shapes are tiny: 3 envs (less than a workgroup's four waves), 64, and 300 (many workgroups,
the last one partly empty)."""
import gc
import json
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest
import torch

from keisei_amd import _lib
from keisei_amd import shogi_gym as G
from keisei_amd.shogi_gym import (ACTION_SPACE, DEFAULT_ACTION_SPACE, SpatialActionMapper, DefaultActionMapper, VecEnv,
                                  hodges_notation, host_move_note, move_usi, start_pool_index)
from keisei_amd.training import LeagueRollout, MatchArena, SelfPlayRollout
from keisei_amd.training.katago_ppo import KataGoRolloutBuffer
from keisei_amd.training.model_group import SEResNetGroup
from keisei_amd.training.models.se_resnet import SEResNetModel, SEResNetParams
from oracle import keisei_oracle as orc
from oracle import shogi as so
from start_pool_helpers import START, mate_in_one

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPE = orc.NetShape(2, 128, 8, 64, 16, 128, 64)                 # the smallest tower the device group covers (128 channels)
OBS = (50, 9, 9)
SENTINEL = -0x5A5A5A5B
TYPES = {"P": 1, "L": 2, "N": 3, "S": 4, "G": 5, "B": 6, "R": 7, "K": 8}
_MODELS = {}


@pytest.fixture(autouse=True)
def _release_device_objects():
    """(see tests/test_hip_selfplay_rollout.py: rollout objects own captured graphs and pinned buffers)"""
    yield
    gc.collect()
    torch.cuda.synchronize()
    gc.collect()


def _model(salt=7):
    if salt not in _MODELS:
        m = SEResNetModel(SEResNetParams(**SHAPE.__dict__))
        m.load_state_dict(orc.init_like_state_dict(SHAPE, salt=salt), strict=True)
        _MODELS[salt] = m.to(DEV).eval()
    return _MODELS[salt]


def _pack(mask: np.ndarray) -> np.ndarray:
    """bool rows -> packed rows (bit j of word w = action 32 w + j)"""
    n, A = mask.shape
    pad = np.zeros((n, (-A) % 32), bool)
    return np.packbits(np.concatenate([mask.astype(bool), pad], axis=1), axis=1, bitorder="little").view(np.uint32)


def _guard_hist(env):
    """Move the env's history rows into the middle of a larger tensor of sentinels (before any step is captured)."""
    n, L = env._hist.shape
    big = torch.full((n + 4, L), SENTINEL, dtype=torch.int32, device=DEV)
    env._hist = big[2:2 + n]
    return big


def _guards_intact(big) -> bool:
    b = big.cpu().numpy()
    return bool((b[:2] == SENTINEL).all() and (b[-2:] == SENTINEL).all())


# ------------------------------------------------------------------ layout
def test_words_match_the_python_layout():
    names = ("NOTE_ACTION_BITS", "NOTE_COLOUR", "NOTE_TYPE", "NOTE_PROMOTED", "NOTE_DROP", "NOTE_CAPTURE", "NOTE_SUFFIX",
             "NOTE_DISAMB", "NOTE_NO_PIECE", "NOTE_WORDS")
    assert [_lib.query("ka_spectator_words", i) for i in range(len(names))] == [getattr(G, n) for n in names]
    assert _lib.query("ka_spectator_words", len(names)) == -1


# ------------------------------------------------------------------ the dicts of a default-constructed env
def test_get_spectator_data_of_a_default_env():
    env = VecEnv(4, 50, "katago", "spatial")
    r = env.reset()
    data = env.get_spectator_data()
    assert isinstance(data, list) and len(data) == 4
    for i, d in enumerate(data):
        assert set(d) == {"board", "hands", "current_player", "ply", "is_over", "result", "sfen", "in_check", "move_history"}
        assert d["current_player"] == "black" and d["ply"] == 0 and d["is_over"] is False and d["result"] == "in_progress"
        assert d["in_check"] is False and len(d["board"]) == 81 and d["hands"]["black"]["pawn"] == 0
        assert d["sfen"] == env.get_sfen(i) == START and d["move_history"] == []
    env.step([int(np.flatnonzero(m)[0]) for m in r.legal_masks])
    data = env.get_spectator_data()
    for i, d in enumerate(data):
        assert d["ply"] == 1 and d["current_player"] == "white" and d["move_history"] == []
        assert d["sfen"] == env.get_sfen(i) != START
    assert env.get_spectator_data([2]) == data[2:3] and env.get_spectator_data([3, 0]) == [data[3], data[0]]
    with pytest.raises(IndexError):
        env.get_spectator_data([4])
    assert not env.move_history and env._hist is None and env._hist_count is None and env._hist_pending is None
    json.dumps(data)


# ------------------------------------------------------------------ device notes against the host restatement
@pytest.mark.parametrize("mode", ["spatial", "default"])
@pytest.mark.parametrize("E", [3, 64, 300])
def test_histories_equal_the_host_notes_in_lockstep_with_the_oracle(E, mode):
    max_ply, plies = 24, 60
    env = VecEnv(E, max_ply, "katago", mode, move_history=True)
    big = _guard_hist(env)
    ref = so.OracleVecEnv(E, max_ply, "katago", mode)
    r0, (_, mask) = env.reset(), ref.reset()
    assert np.array_equal(r0.legal_masks, mask)
    rng = np.random.default_rng(11 + E)
    want = [[] for _ in range(E)]
    finished = np.zeros(E, int)
    assert all(len(h) == 0 for h in env.move_notes())
    for ply in range(plies):
        acts = np.array([rng.choice(np.flatnonzero(m)) for m in mask], np.int64)
        bits = _pack(mask)
        for e in range(E):
            board, _, side, _ = ref.state(e)
            want[e].append(host_move_note(board, side, bits[e], int(acts[e]), mode))
        rd, rr = env.step(acts), ref.step(acts)
        assert np.array_equal(rd.legal_masks, rr["legal_masks"])
        done = rr["terminated"] | rr["truncated"]
        assert np.array_equal(done, rd.terminated | rd.truncated)
        for e in np.flatnonzero(done):
            want[e] = []
            finished[e] += 1
        got = env.move_notes()
        for e in range(E):
            assert got[e].tolist() == want[e], (ply, e)       # (empty right after the env finished)
        mask = rr["legal_masks"]
    assert finished.min() >= 2 and _guards_intact(big)
    assert int(env._hist_count.max()) <= max_ply
    some = env.get_spectator_data([0, E - 1])
    for d, e in zip(some, (0, E - 1)):
        assert [m["action"] for m in d["move_history"]] == [n & 0x3FFF for n in want[e]]
        assert [m["notation"] for m in d["move_history"]] == [hodges_notation(n, mode) for n in want[e]]
    env.reset()
    assert all(len(h) == 0 for h in env.move_notes())


# ------------------------------------------------------------------ a game that ends by checkmate
def test_checkmate_clears_the_history_of_that_env_only():
    board, hands, side, mate = mate_in_one()
    start = G.parse_sfen(START)
    N = 4
    seed = next(s for s in range(100) if (start_pool_index(s, np.arange(N), 0, 2) == 1).sum() == 1)
    e_mate = int(np.flatnonzero(start_pool_index(seed, np.arange(N), 0, 2) == 1)[0])
    env = VecEnv(N, 200, "katago", "spatial", start_pool_capacity=2, move_history=True)
    env.set_start_positions(np.stack([start[0], board]), np.stack([start[1], hands]), np.array([start[2], side]), seed=seed)
    r = env.reset()
    acts = np.array([int(np.flatnonzero(m)[0]) for m in r.legal_masks], np.int64)
    assert r.legal_masks[e_mate, mate]
    acts[e_mate] = mate
    r = env.step(acts)
    assert r.terminated[e_mate] and r.step_metadata.termination_reason[e_mate] == so.R_CHECKMATE and r.terminated.sum() == 1
    notes = env.move_notes()
    assert len(notes[e_mate]) == 0
    for e in range(N):
        if e != e_mate:
            assert [n & 0x3FFF for n in notes[e].tolist()] == [int(acts[e])]
    acts2 = np.array([int(np.flatnonzero(m)[0]) for m in r.legal_masks], np.int64)
    env.step(acts2)
    after = env.move_notes()
    for e in range(N):
        assert [n & 0x3FFF for n in after[e].tolist()] == ([int(acts2[e])] if e == e_mate else [int(acts[e]), int(acts2[e])])
        assert after[e][:len(notes[e])].tolist() == notes[e].tolist()


# ------------------------------------------------------------------ constructed positions
@lru_cache(maxsize=None)
def _vectors():
    doc = json.loads((Path(__file__).resolve().parent / "golden" / "g16_spectator_vectors.json").read_text())
    return [v for v in doc["vectors"] if v["kings"] is not None]


def _vector_state(v):
    b = np.zeros(81, np.uint8)
    for r, c, t, col, prom in v["pieces"]:
        b[r * 9 + c] = TYPES[t] | (0x10 if col == "white" else 0) | (0x20 if prom else 0)
    for col, (r, c) in v["kings"].items():
        b[r * 9 + c] = 8 | (0x10 if col == "white" else 0)
    return b, np.array([v["hands"]["black"], v["hands"]["white"]], np.uint8), v["side"]


def _vector_action(v, spatial: bool) -> int:
    mapper, m = (SpatialActionMapper() if spatial else DefaultActionMapper()), v["move"]
    to = m["to"][0] * 9 + m["to"][1]
    if "drop" in m:
        return mapper.encode_drop_move(to, "PLNSGBR".index(m["drop"]), bool(v["side"]))
    return mapper.encode_board_move(m["from"][0] * 9 + m["from"][1], to, bool(m["promote"]), bool(v["side"]))


@pytest.mark.parametrize("mode", ["spatial", "default"])
def test_constructed_positions_give_the_fixture_strings(mode):
    vs = _vectors()
    assert len(vs) >= 30 and sum(v["name"].startswith("three_silvers") for v in vs) == 6
    states = [_vector_state(v) for v in vs]
    env = VecEnv(len(vs), 100, "katago", mode, move_history=True)
    env.reset()
    env.set_states(np.stack([s[0] for s in states]), np.stack([s[1] for s in states]), np.array([s[2] for s in states]))
    acts = np.array([_vector_action(v, mode == "spatial") for v in vs], np.int64)
    env.step(acts)
    for v, a, d in zip(vs, acts, env.get_spectator_data()):
        assert d["move_history"] == [{"action": int(a), "notation": v["hodges"], "usi": v["usi"]}], v["name"]


# ------------------------------------------------------------------ refused steps
def test_a_refused_step_changes_no_history():
    N = 5
    env = VecEnv(N, 100, "katago", "spatial", check_actions=False, move_history=True)
    big = _guard_hist(env)
    r = env.reset()
    first = np.array([int(np.flatnonzero(m)[0]) for m in r.legal_masks], np.int64)
    r = env.step(first)
    env.raise_if_refused()
    before = [h.tolist() for h in env.move_notes()]
    assert [len(h) for h in before] == [1] * N
    legal = np.array([int(np.flatnonzero(m)[-1]) for m in r.legal_masks], np.int64)
    bad = legal.copy()
    bad[2] = int(np.flatnonzero(~r.legal_masks[2])[0])           # inside the action space, not legal
    r2 = env.step(bad)
    assert [h.tolist() for h in env.move_notes()] == before
    with pytest.raises(RuntimeError, match=f"env 2: action index {bad[2]} is not legal"):
        env.raise_if_refused()
    assert np.array_equal(r2.legal_masks, r.legal_masks)         # the unchanged positions
    neg = legal.copy()
    neg[1] = -3
    env.step(neg)
    assert [h.tolist() for h in env.move_notes()] == before
    with pytest.raises(ValueError, match="env 1: negative action index -3"):
        env.raise_if_refused()
    env.step(legal)
    env.raise_if_refused()
    after = [h.tolist() for h in env.move_notes()]
    assert [h[:1] for h in after] == before and [h[1] & 0x3FFF for h in after] == legal.tolist()
    assert [len(h) for h in after] == [2] * N and _guards_intact(big)


@pytest.mark.parametrize("mode,A", [(1, ACTION_SPACE), (0, DEFAULT_ACTION_SPACE)])
def test_an_action_outside_the_action_space_reads_and_writes_nothing_out_of_bounds(mode, A):
    """The note launch alone over guard-banded buffers: mask rows between 0xFF rows (a read behind a row would find
    'others' everywhere), pending between sentinels.  Actions outside [0, A) give note 0; the legal ones beside them
    their host note."""
    E, words = 6, (A + 31) // 32
    ref = so.OracleVecEnv(E, 100, "katago", "spatial" if mode else "default")
    _, mask = ref.reset()
    acts = np.array([A, int(np.flatnonzero(mask[1])[3]), -1, A + 40, 1 << 40, int(np.flatnonzero(mask[5])[-1])], np.int64)
    state = np.zeros((E + 2, 128), np.uint8)
    state[[0, -1]] = 0xFF
    for e in range(E):
        board, hands, side, _ = ref.state(e)
        state[1 + e, :81], state[1 + e, 81:95], state[1 + e, 95] = board, hands.reshape(14), side
    bits = np.full((E + 2, words), 0xFFFFFFFF, np.uint32)
    bits[1:-1] = _pack(mask)
    pending = np.full(E + 2, SENTINEL, np.int32)
    d_state, d_bits = torch.from_numpy(state).to(DEV), torch.from_numpy(bits.view(np.int32)).to(DEV)
    d_pending, d_acts = torch.from_numpy(pending).to(DEV), torch.from_numpy(acts).to(DEV)
    _lib.call("ka_spectator_note", d_state[1:-1], 128, E, d_bits[1:-1], d_acts, mode, d_pending[1:-1], _lib.stream_ptr())
    torch.cuda.synchronize()
    got = d_pending.cpu().numpy()
    assert got[0] == SENTINEL and got[-1] == SENTINEL
    assert np.array_equal(d_bits.cpu().numpy().view(np.uint32), bits) and np.array_equal(d_state.cpu().numpy(), state)
    board = state[1, :81]
    want = [0, host_move_note(board, 0, bits[2], int(acts[1]), mode), 0, 0, 0, host_move_note(board, 0, bits[6], int(acts[5]), mode)]
    assert got[1:-1].tolist() == want and want[1] != 0 and want[5] != 0


# ------------------------------------------------------------------ inside captured plies
def _rollout_feed(graph, sync_every, move_history=True):
    N, plies = 64, 32
    roll = SelfPlayRollout(_model(), num_envs=N, max_ply=12, graph=graph, sync_every=sync_every, seed=5, game_log=64,
                           move_history=move_history)
    buf = KataGoRolloutBuffer(N, OBS, ACTION_SPACE, device=DEV)
    roll.collect(buf, plies)
    data, live = roll.spectator_data(), roll.live_games()
    values = roll.last_values.cpu().numpy()
    return roll, data, live, values


def test_histories_inside_captured_plies_agree_with_the_game_log():
    runs = [_rollout_feed(True, 8), _rollout_feed(False, 2)]
    assert runs[0][1] == runs[1][1]
    for roll, data, live, values in runs:
        assert len(data) == len(live) == 64 and roll.env.move_history
        assert sum(len(d["move_history"]) for d in data) > 64
        for e, (d, g) in enumerate(zip(data, live)):
            assert g.env == e and not g.finished
            assert [m["action"] for m in d["move_history"]] == g.actions.tolist()
            assert [m["usi"] for m in d["move_history"]] == g.usi_moves()
            assert d["ply"] == len(g.actions) and d["value_estimate"] == float(values[e])
        assert roll.spectator_data([5, 1]) == [data[5], data[1]]
        json.dumps(data)


def test_without_move_history_the_rollout_feed_has_empty_histories_and_no_buffers():
    roll, data, live, _ = _rollout_feed(True, 8, move_history=False)
    env = roll.env
    assert not env.move_history and env._hist is None and env._hist_count is None and env._hist_pending is None
    assert len(data) == 64 and all(d["move_history"] == [] and "value_estimate" in d for d in data)
    assert [d["ply"] for d in data] == [len(g.actions) for g in live]
    assert [d["sfen"] for d in data] == env.get_sfens()


def test_league_rollout_and_arena_hand_out_the_feed():
    league = LeagueRollout(_model(1), [_model(2)], [10], num_envs=8, max_ply=12, graph=True, sync_every=4, seed=3,
                           move_history=True, game_log=16)
    buf = KataGoRolloutBuffer(8, OBS, ACTION_SPACE, device=DEV)
    league.collect(buf, 8)
    data, live = league.spectator_data(), league.live_games()
    for d, g in zip(data, live):
        assert [m["action"] for m in d["move_history"]] == g.actions.tolist() and "value_estimate" not in d
        assert [m["usi"] for m in d["move_history"]] == g.usi_moves()
    arena = MatchArena(SEResNetGroup([_model(1), _model(2)]), num_envs=8, envs_per_match=4, max_ply=12, sync_every=4, seed=3,
                       move_history=True, game_log=16)
    arena.run_round([(0, 1)], games_per_match=4)
    data, live = arena.spectator_data(), arena.live_games()
    assert len(data) == 8
    for d, g in zip(data, live):
        assert [m["action"] for m in d["move_history"]] == g.actions.tolist()
        assert [m["usi"] for m in d["move_history"]] == g.usi_moves()
