"""The game log kernels (ka_gamelog_begin / ka_gamelog_step / ka_gamelog_seat) against their numpy restatement
(keisei_amd.training.game_log.HostGameLog) on synthetic plies: no model and no env, a fake state array with random start
positions, random actions and done flags.  Records, cursor, move rows, start slots and counters are compared bit for bit
after every ply; a guard record behind the log and a sentinel behind every move row catch a write out of bounds."""
import numpy as np
import pytest
import torch

from keisei_amd import _lib
from keisei_amd.training.game_log import CURSOR_WORDS, META_WORDS, START_WORDS, HostGameLog, record_words

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAX_PLY, PLIES = 6, 12
PATTERN = 0x7FC0A5A5
TILE = 256                                                       # envs one pass of the step kernel's workgroup covers


def _plies(E, n, seed, *, done_rate=0.25, live_rate=None, stall=False):
    rng = np.random.default_rng(seed)
    out = []
    for t in range(n):
        tm = rng.random(E) < done_rate / 2
        tr = rng.random(E) < done_rate / 2
        rewards = np.where(tm, rng.choice(np.asarray([-1.0, 0.0, 1.0], np.float32), E), np.float32(0)).astype(np.float32)
        ply = dict(state=rng.integers(0, 256, (E, _lib.query("ka_shogi_env_state_bytes")), dtype=np.uint8),
                   actions=rng.integers(0, 11259, E, dtype=np.int64), rewards=rewards, terminated=tm, truncated=tr,
                   pre_players=rng.integers(0, 2, E, dtype=np.uint8), reason=rng.integers(0, 6, E, dtype=np.uint8),
                   ply_counter=1000 + 3 * t)
        if live_rate is not None:
            ply["live"] = np.where(rng.random(E) < live_rate, -1, rng.integers(0, 4, E)).astype(np.int32)
        if stall:
            ply["n_legal"] = np.where(rng.random(E) < 0.08, 0, rng.integers(1, 90, E)).astype(np.int32)
        out.append(ply)
    return out


def _drive(E, plies, *, cap, max_ply=MAX_PLY, pairs=None, pair_stride=0, envs_per_pair=1, seats=None, slots=0,
           envs_per_slot=0, sentinel=2):
    """Run the plies through the kernels and through HostGameLog, comparing every buffer after every ply.  ``seats``:
    {ply index: jobs (n, 4) int32}, applied before that ply.  Returns the host log."""
    words, stride = record_words(max_ply), 2 * ((max_ply + 1) // 2) + sentinel
    host = HostGameLog(E, max_ply, cap + 1, row_stride=stride, fill=PATTERN)      # one guard record behind the log
    host.capacity = cap
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    rows = t(host.rows.view(np.int16))
    meta = torch.full((E, META_WORDS), 77, dtype=torch.int32, device=DEV)         # begin clears them
    starts = torch.zeros(E, START_WORDS, dtype=torch.int32, device=DEV)
    records = t(host.records)
    cursor = torch.zeros(CURSOR_WORDS, dtype=torch.int32, device=DEV)
    pairs_d = t(np.asarray(pairs, np.int32)) if pairs is not None else None
    ply_word = torch.zeros(1, dtype=torch.int32, device=DEV)
    st = _lib.stream_ptr()
    first = plies[0]["state"].copy()
    state = t(first)
    sb = int(state.shape[1])
    _lib.call("ka_gamelog_begin", state, sb, E, meta, starts, st)
    host.begin(first)

    def same(when):
        for name, dev_t, ref in (("rows", rows, host.rows.view(np.int16)), ("meta", meta, host.meta), ("starts", starts, host.starts),
                                 ("records", records, host.records), ("cursor", cursor, host.cursor)):
            got = dev_t.cpu().numpy()
            assert np.array_equal(got, ref), f"{name} differ {when}: first at {np.argwhere(got != ref)[:4].tolist()}"

    same("after begin")
    for i, p in enumerate(plies):
        if seats and i in seats:
            jobs = np.asarray(seats[i], np.int32)
            _lib.call("ka_gamelog_seat", t(jobs), len(jobs), slots, envs_per_slot, meta, st)
            host.seat(jobs, slots, envs_per_slot)
        state.copy_(t(p["state"]))
        ply_word.fill_(p["ply_counter"])
        _lib.call("ka_gamelog_step", state, sb, E, max_ply, t(p["actions"]), t(p["rewards"]), t(p["terminated"]),
                  t(p["truncated"]), t(p["pre_players"]), t(p["reason"]), t(p["n_legal"]) if "n_legal" in p else None,
                  t(p["live"]) if "live" in p else None, pairs_d, pair_stride, envs_per_pair, ply_word, rows, stride, meta,
                  starts, records, cap, cursor, st)
        host.step(p["state"], p["actions"], p["rewards"], p["terminated"], p["truncated"], p["pre_players"], p["reason"],
                  nlegal=p.get("n_legal"), live=p.get("live"), pairs=pairs, pair_stride=pair_stride,
                  envs_per_pair=envs_per_pair, ply_counter=p["ply_counter"])
        same(f"after ply {i}")
    assert (host.records[cap] == np.int32(PATTERN)).all()         # (and so is the device's: `same` compared it)
    assert (host.rows[:, stride - sentinel:] == PATTERN & 0xFFFF).all()
    return host


@pytest.mark.parametrize("E", [1, 5, 65, 2 * TILE + 3])
def test_step_matches_the_host_restatement(E):
    """Below one wave, one past a wave, across two tiles of the workgroup plus three: the places a rank can go wrong."""
    host = _drive(E, _plies(E, PLIES, seed=E), cap=E * PLIES)
    n = int(host.cursor[0])
    assert host.cursor[1] == 0 and host.cursor[2] == PLIES
    if E >= 5:
        assert n > 0
    games = host.games()
    assert [g.end_ply for g in games] == sorted(g.end_ply for g in games)        # (ply, env) order
    assert all(a.env < b.env for a, b in zip(games, games[1:]) if a.end_ply == b.end_ply)
    assert all(1 <= len(g.actions) <= MAX_PLY for g in games)


def test_live_envs_and_a_seat_call():
    E, eps = 65, 5
    jobs = [[0, 1, 2, 4], [7, 0, 3, 4], [12, 2, 2, 4], [13, 0, 0, 4], [-1, 0, 0, 4]]      # the last two name no slot
    host = _drive(E, _plies(E, PLIES, seed=11, live_rate=1 / 3), cap=E * PLIES, seats={6: jobs}, slots=E // eps, envs_per_slot=eps)
    games = host.games()
    assert any(g.carried for g in games) and any(not g.carried for g in games)
    assert 0 < len(games) < host.meta[:, 2].sum()                # finished games of envs that were not live are skipped


def test_pair_table_and_stalled_groups():
    E = 12
    pairs = np.arange(24, dtype=np.int32).reshape(3, 8) + 100     # stride 8: the arena's slot rows {model_a, model_b, ...}
    host = _drive(E, _plies(E, PLIES, seed=5, stall=True), cap=E * PLIES, pairs=pairs, pair_stride=8, envs_per_pair=4)
    games = host.games()
    assert games and all((g.black, g.white) == (100 + 8 * (g.env // 4), 101 + 8 * (g.env // 4)) for g in games)
    assert len(games) < host.meta[:, 2].sum()                    # a group with an env without a legal action commits nothing


def test_games_beyond_the_capacity_are_dropped_whole():
    E, cap = 65, 7
    host = _drive(E, _plies(E, PLIES, seed=3), cap=cap)
    assert host.cursor[0] == cap and host.cursor[1] == host.meta[:, 2].sum() - cap > 0


def test_a_move_row_is_never_written_past_max_ply():
    E = 5
    plies = _plies(E, MAX_PLY + 3, seed=9, done_rate=0.0)
    plies[-1]["truncated"][:] = True
    host = _drive(E, plies, cap=E)
    games = host.games()
    assert len(games) == E and all(len(g.actions) == MAX_PLY for g in games)
    for e, g in enumerate(games):
        assert g.actions.tolist() == [int(p["actions"][e]) for p in plies[:MAX_PLY]]


def test_odd_max_ply_pads_the_last_move_word():
    E, max_ply = 5, 5
    plies = _plies(E, 10, seed=13, done_rate=0.3)
    _drive(E, plies, cap=E * 10, max_ply=max_ply)
