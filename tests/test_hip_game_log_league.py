"""The game log with per-env players on the device: ka_gamelog_step_env and ka_gamelog_peek against their numpy
restatement (HostGameLog) word for word on synthetic plies, the existing entry on the same plies, and the log inside
LeagueRollout -- the drained games against the host log run over the rollout's own per-ply record, every game replayed on
the CPU oracle, the schedule and the log leaving the epoch unchanged, a new cohort in the middle of a run, the games in
progress, and the way back to SL data."""
import gc

import numpy as np
import pytest
import torch

from keisei_amd import _lib
from keisei_amd.shogi_gym import ACTION_SPACE
from keisei_amd.sl.prepare import dataset_from_recorded_games
from keisei_amd.training import LeagueRollout, MatchArena, SelfPlayRollout, game_log_host
from keisei_amd.training.game_log import HostGameLog, games_from_records, record_words
from keisei_amd.training.katago_ppo import KataGoRolloutBuffer
from keisei_amd.training.model_group import SEResNetGroup
from keisei_amd.training.models.se_resnet import SEResNetModel, SEResNetParams
from keisei_amd.training.value_adapter import MultiHeadValueAdapter
from oracle import keisei_oracle as orc
from oracle import shogi as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
PATTERN = -0x5A5A5A5B                                            # 0xA5A5A5A5 as int32
PLIES = 20


@pytest.fixture(autouse=True)
def _release_device_objects():
    yield
    gc.collect()
    torch.cuda.synchronize()
    gc.collect()


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------------------------------------- synthetic plies
def _plies(E, K, seed, n=PLIES):
    """Random plies with forced terminations and truncations, side / opponent changes per ply (some indices outside [0, K),
    one that wraps the tag's shift), envs without a legal action, and fresh random state rows every ply."""
    rng = np.random.default_rng(seed)
    sb = _lib.query("ka_shogi_env_state_bytes")
    side = rng.integers(0, 2, E, dtype=np.uint8)
    opp = rng.integers(0, K, E).astype(np.int32)
    odd = np.asarray([-1, K, K + 5, -7, 0x7FFFFFFF, -0x80000000], np.int32)
    out = []
    for t in range(n):
        flip = rng.random(E) < 0.12
        side = np.where(flip, 1 - side, side).astype(np.uint8)
        move = rng.random(E) < 0.12
        opp = np.where(move, rng.integers(0, K, E), opp).astype(np.int32)
        wild = rng.random(E) < 0.04
        opp = np.where(wild, rng.choice(odd, E), opp).astype(np.int32)
        tm = rng.random(E) < 0.12
        tr = rng.random(E) < 0.12
        if t in (4, 11):
            tm[:] = True                                         # every env at once: ranks across all waves and tiles
        if t == 15:
            tr[:] = True
        rewards = np.where(tm, rng.choice(np.asarray([-1.0, 0.0, 1.0], np.float32), E), np.float32(0)).astype(np.float32)
        out.append(dict(state=rng.integers(0, 256, (E, sb), dtype=np.uint8), actions=rng.integers(0, 11259, E, dtype=np.int64),
                        rewards=rewards, terminated=tm, truncated=tr, pre_players=rng.integers(0, 2, E, dtype=np.uint8),
                        reason=rng.integers(0, 6, E, dtype=np.uint8), ply_counter=500 + 7 * t,
                        n_legal=np.where(rng.random(E) < 0.05, 0, rng.integers(1, 90, E)).astype(np.int32),
                        side=side.copy(), opp=opp.copy()))
    return out


class _Pair:
    """The device buffers of one log beside a HostGameLog over the same words: every buffer starts as 0xA5 bytes (begin
    clears what it owns), one guard record lies behind the log and two sentinel moves behind every row."""

    def __init__(self, E, max_ply, cap, first_state):
        self.E, self.max_ply, self.cap = E, max_ply, cap
        self.stride = 2 * ((max_ply + 1) // 2) + 2
        self.host = HostGameLog(E, max_ply, cap + 1, row_stride=self.stride, fill=PATTERN)
        self.host.capacity = cap
        self.host.meta[:] = PATTERN
        self.host.starts[:] = PATTERN
        self.host.cursor[:] = 0                                  # the owner zeroes the cursor, not begin
        self.rows = _t(self.host.rows.view(np.int16))
        self.meta, self.starts = _t(self.host.meta), _t(self.host.starts)
        self.records, self.cursor = _t(self.host.records), _t(self.host.cursor)
        self.state = _t(first_state)
        self.sb = int(self.state.shape[1])
        self.ply_word = torch.zeros(1, dtype=torch.int32, device=DEV)
        _lib.call("ka_gamelog_begin", self.state, self.sb, E, self.meta, self.starts, _lib.stream_ptr())
        self.host.begin(first_state)
        self.same("after begin")

    def buffers(self):
        return [t.cpu().numpy().copy() for t in (self.rows, self.meta, self.starts, self.records, self.cursor)]

    def same(self, when):
        h = self.host
        for name, got, ref in zip(("rows", "meta", "starts", "records", "cursor"), self.buffers(),
                                  (h.rows.view(np.int16), h.meta, h.starts, h.records, h.cursor)):
            assert np.array_equal(got, ref), f"{name} differ {when}: first at {np.argwhere(got != ref)[:4].tolist()}"

    def step_env(self, p, ids, ids_d, K):
        self.state.copy_(_t(p["state"]))
        self.ply_word.fill_(p["ply_counter"])
        _lib.call("ka_gamelog_step_env", self.state, self.sb, self.E, self.max_ply, _t(p["actions"]), _t(p["rewards"]),
                  _t(p["terminated"]), _t(p["truncated"]), _t(p["pre_players"]), _t(p["reason"]), _t(p["n_legal"]), None,
                  _t(p["side"]), _t(p["opp"]), ids_d, K, self.ply_word, self.rows, self.stride, self.meta, self.starts,
                  self.records, self.cap, self.cursor, _lib.stream_ptr())
        self.host.step(p["state"], p["actions"], p["rewards"], p["terminated"], p["truncated"], p["pre_players"], p["reason"],
                       nlegal=p["n_legal"], side=p["side"], opp=p["opp"], ids=ids, ply_counter=p["ply_counter"])

    def step_pairs(self, p, pairs, pairs_d, stride, per):
        self.state.copy_(_t(p["state"]))
        self.ply_word.fill_(p["ply_counter"])
        _lib.call("ka_gamelog_step", self.state, self.sb, self.E, self.max_ply, _t(p["actions"]), _t(p["rewards"]),
                  _t(p["terminated"]), _t(p["truncated"]), _t(p["pre_players"]), _t(p["reason"]), _t(p["n_legal"]), None,
                  pairs_d, stride, per, self.ply_word, self.rows, self.stride, self.meta, self.starts, self.records,
                  self.cap, self.cursor, _lib.stream_ptr())
        self.host.step(p["state"], p["actions"], p["rewards"], p["terminated"], p["truncated"], p["pre_players"], p["reason"],
                       nlegal=p["n_legal"], pairs=pairs, pair_stride=stride, envs_per_pair=per, ply_counter=p["ply_counter"])

    def guards_hold(self):
        assert (self.host.records[self.cap] == np.int32(PATTERN)).all()          # (and the device's: `same` compared it)
        assert (self.host.rows[:, self.stride - 2:] == PATTERN & 0xFFFF).all()


def _ids(K):
    return np.asarray([1000] + [10 * k + 3 for k in range(K)], np.int32)


@pytest.mark.parametrize("max_ply, K", [(5, 1), (6, 3)], ids=["max_ply5-K1", "max_ply6-K3"])
@pytest.mark.parametrize("E", [1, 63, 64, 65, 256, 257, 300])
def test_step_env_matches_the_host_restatement(E, max_ply, K):
    """One env, the wave boundary (63 / 64 / 65) and the workgroup's 256-env tile boundary (256 / 257 / 300)."""
    plies = _plies(E, K, seed=100 * E + K)
    cap = 5 * E                                                   # more than six games per env finish: the log fills up
    pair = _Pair(E, max_ply, cap, plies[0]["state"])
    ids = _ids(K)
    ids_d = _t(ids)
    for i, p in enumerate(plies):
        pair.step_env(p, ids, ids_d, K)
        pair.same(f"after ply {i}")
    pair.guards_hold()
    h = pair.host
    assert h.cursor[0] == cap and h.cursor[1] > 0 and h.cursor[2] == PLIES
    games = h.games()
    assert all(g.learner_side in (0, 1) and g.finished for g in games)
    if E >= 63:
        assert any(g.carried for g in games) and any(not g.carried for g in games)
        assert any(-1 in (g.black, g.white) for g in games) == any(not 0 <= int(p["opp"][g.env]) < K for g in games
                                                                   for p in plies if p["ply_counter"] == g.end_ply)
    for g in games:
        me = g.white if g.learner_side else g.black
        assert me == 1000 and (g.black if g.learner_side else g.white) in (-1, *ids[1:].tolist())


def test_the_existing_entry_is_where_it_was():
    """ka_gamelog_step on the same plies, players from a pair table: the host restatement of the parent, and the fourth meta
    word, which only the per-env entry owns, is never written."""
    E, max_ply = 257, 6
    plies = _plies(E, 3, seed=77)
    pair = _Pair(E, max_ply, 5 * E, plies[0]["state"])
    pair.meta[:, 3] = 77
    pair.host.meta[:, 3] = 77
    groups = (E + 3) // 4
    pairs = (np.arange(8 * groups, dtype=np.int32).reshape(groups, 8) + 100)
    pairs_d = _t(pairs)
    for i, p in enumerate(plies):
        pair.step_pairs(p, pairs, pairs_d, 8, 4)
        pair.same(f"after ply {i}")
    pair.guards_hold()
    assert (pair.meta[:, 3].cpu().numpy() == 77).all()
    n = int(pair.host.cursor[0])
    assert n > 0 and (pair.host.records[:n, 9] == 0).all()
    assert all(g.learner_side is None and (g.black, g.white) == (100 + 8 * (g.env // 4), 101 + 8 * (g.env // 4))
               for g in pair.host.games())


@pytest.mark.parametrize("E, max_ply, K", [(65, 5, 3), (300, 6, 1)])
def test_peek_matches_the_host_restatement_and_writes_nothing_else(E, max_ply, K):
    plies = _plies(E, K, seed=5 * E)
    pair = _Pair(E, max_ply, 2 * E, plies[0]["state"])
    ids = _ids(K)
    ids_d = _t(ids)
    for p in plies[:11]:                                          # six plies behind the ply that finished every env
        pair.step_env(p, ids, ids_d, K)
    pair.same("before the peek")
    before = pair.buffers()
    nxt = plies[11]
    side_d, opp_d = _t(nxt["side"]), _t(nxt["opp"])
    pair.ply_word.fill_(4321)
    words = record_words(max_ply)
    groups = (E + 3) // 4
    pairs = (np.arange(8 * groups, dtype=np.int32).reshape(groups, 8) + 100)
    pairs_d = _t(pairs)
    picks = np.asarray([E - 1, 0, E, 3 % E, -1, 0, E - 1, 1 << 20, 0], np.int32)
    assert pair.host.meta[:, 0].max() == max_ply                  # some rows are full
    for lst in (None, picks):
        n = E if lst is None else len(lst)
        lst_d = None if lst is None else _t(lst)
        for who in ("env", "pairs", "nobody"):
            out = torch.full((n + 2, words), PATTERN, dtype=torch.int32, device=DEV)          # a guard row on either side
            want = np.full((n, words), PATTERN, np.int32)
            dev_kw = (None, 0, 1, None, None, None, 0)
            host_kw = {}
            if who == "env":
                dev_kw, host_kw = (None, 0, 1, side_d, opp_d, ids_d, K), dict(side=nxt["side"], opp=nxt["opp"], ids=ids)
            elif who == "pairs":
                dev_kw, host_kw = (pairs_d, 8, 4, None, None, None, 0), dict(pairs=pairs, pair_stride=8, envs_per_pair=4)
            _lib.call("ka_gamelog_peek", lst_d, n, E, max_ply, *dev_kw, pair.ply_word, pair.rows, pair.stride, pair.meta,
                      pair.starts, out[1:], _lib.stream_ptr())
            pair.host.peek(lst, ply_counter=4321, out=want, **host_kw)
            got = out.cpu().numpy()
            assert (got[0] == PATTERN).all() and (got[-1] == PATTERN).all()
            assert np.array_equal(got[1:-1], want), (who, np.argwhere(got[1:-1] != want)[:4].tolist())
            valid = [j for j in range(n) if lst is None or 0 <= lst[j] < E]
            games = games_from_records(want[valid])
            assert all(not g.finished and g.winner == -1 and g.end_ply == 4321 for g in games)
            if lst is None:
                assert any(len(g.actions) % 2 for g in games) and any(len(g.actions) == max_ply for g in games)
    for b, a in zip(before, pair.buffers()):
        assert np.array_equal(a, b)
    pair.guards_hold()
    with pytest.raises(_lib.KeiseiHipError, match="not both"):
        _lib.call("ka_gamelog_peek", None, E, E, max_ply, pairs_d, 8, 4, side_d, opp_d, ids_d, K, None, pair.rows, pair.stride,
                  pair.meta, pair.starts, out, _lib.stream_ptr())
    with pytest.raises(_lib.KeiseiHipError, match="without a list"):
        _lib.call("ka_gamelog_peek", None, E + 1, E, max_ply, None, 0, 1, None, None, None, 0, None, pair.rows, pair.stride,
                  pair.meta, pair.starts, out, _lib.stream_ptr())


# ---------------------------------------------------------------------------------------------- LeagueRollout
SHAPE = orc.NetShape(2, 128, 8, 64, 16, 128, 64)                 # the model of tests/test_hip_league_rollout.py
OBS = (50, 9, 9)
N, MAX_PLY, K3 = 64, 12, 3
OPP_IDS = [10 * k + 3 for k in range(K3)]
LEARNER_ID = 900
# 24 plies in two collects: the second one's side re-draw falls in the middle of the games (they end every 12 plies), and
# three plies more, whose side re-draw falls between two games and which leave three moves in every env for live_games()
FIRST, SECOND, THIRD = 10, 14, 3
TOTAL = FIRST + SECOND + THIRD
_MODELS = []


def _models(n):
    while len(_MODELS) < n:
        m = SEResNetModel(SEResNetParams(**SHAPE.__dict__))
        m.load_state_dict(orc.init_like_state_dict(SHAPE, salt=31 * len(_MODELS) + 7), strict=True)
        _MODELS.append(m.to(DEV).eval())
    return _MODELS[:n]


def _roll(game_log, **kw):
    ms = _models(K3 + 1)
    kw.setdefault("graph", False)
    if game_log is not None:
        kw.update(game_log=game_log, learner_id=LEARNER_ID)
    return LeagueRollout(ms[0], ms[1:], OPP_IDS, num_envs=N, max_ply=MAX_PLY, sync_every=4, seed=4242,
                         value_adapter=MultiHeadValueAdapter(score_blend_alpha=0.25), color_randomization=True,
                         opponent_weights=[1.0, 2.0, 1.0], **kw)


def _epochs(game_log, **kw):
    roll = _roll(game_log, **kw)
    buf = KataGoRolloutBuffer(N, OBS, ACTION_SPACE, device=DEV)
    out, records = [], []
    for steps in (FIRST, SECOND, THIRD):
        out.append(roll.collect(buf, steps))
        records += roll.record
    return roll, out, records, {k: v.clone() for k, v in buf.flatten().items()}


_BASE = {}


def _base():
    """The recorded run every rollout test compares against: computed once."""
    if not _BASE:
        roll, stats, records, cols = _epochs(256, record=True)
        live = roll.live_games()
        _BASE.update(stats=stats, records=records, cols=cols, live=live, side=roll._side.cpu().numpy(),
                     opp=roll._opp.cpu().numpy(), some=roll.live_games([5, 5, 63]))
    return _BASE


def _key(g):
    return (g.env, g.actions.tolist(), g.winner, g.reason, g.truncated, g.carried, g.black, g.white, g.end_ply, g.game_number,
            g.start_board.tobytes(), g.start_hands.tobytes(), g.start_side, g.finished, g.learner_side)


def _same_bits(a, b):
    if a.dtype.is_floating_point:                                # NaN cells compare by their bits
        return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))
    return torch.equal(a, b)


def _winner(reward, mover):
    return mover if reward > 0 else (1 - mover if reward < 0 else 2)


def _replays_on_the_oracle(g, max_ply):
    """Every move legal from the game's start; a finished game is over at its last ply and not before, with the recorded
    reason and winner; a game in progress is not over."""
    env = S.OracleVecEnv(1, max_ply)
    env.reset()
    env.set_state(0, g.start_board, g.start_hands, g.start_side)
    for i, a in enumerate(g.actions):
        _, mask = env.observe(0)
        assert mask[int(a)], (g.env, g.game_number, i, int(a))
        r = env.step(np.asarray([int(a)]))
        done = bool(r["terminated"][0] or r["truncated"][0])
        assert done == (g.finished and i == len(g.actions) - 1), (g.env, g.game_number, i)
    if g.finished:
        assert len(g.actions) >= 1
        assert int(r["termination_reason"][0]) == g.reason
        assert bool(r["truncated"][0] and not r["terminated"][0]) == g.truncated
        assert _winner(float(r["rewards"][0]), (g.start_side + len(g.actions) - 1) & 1) == g.winner


def test_league_games_equal_the_host_log_over_the_record_and_replay_on_the_oracle():
    base = _base()
    records = base["records"]
    assert len(records) == TOTAL
    ids = np.asarray([LEARNER_ID, *OPP_IDS], np.int32)
    host = game_log_host(records, num_envs=N, max_ply=MAX_PLY, capacity=1024, ids=ids)
    want = host.games()
    got = [g for st in base["stats"] for g in st.games]
    assert all(st.games_dropped == 0 for st in base["stats"]) and host.cursor[1] == 0
    assert len(got) >= 2 * N
    assert [_key(g) for g in got] == [_key(g) for g in want]
    # the first batch of games spans the second collect's side re-draw: carried exactly where the env's side changed
    changed = records[FIRST]["side"] != records[FIRST - 1]["side"]
    assert changed.any() and not changed.all()
    first = [g for g in got if g.game_number == 0 and g.truncated]
    assert first and all(g.carried == bool(changed[g.env]) for g in first)
    assert not any(g.carried for g in got if g.end_ply - len(g.actions) + 1 >= FIRST)
    # the players: the ones of the game's last ply
    for g in got:
        rec = records[g.end_ply]
        assert g.learner_side == int(rec["side"][g.env])
        assert (g.white if g.learner_side else g.black) == LEARNER_ID
        assert (g.black if g.learner_side else g.white) == OPP_IDS[int(rec["opp"][g.env])]
    # each collect's decided games, by the record's opponent id, are its opponent_results
    for st in base["stats"]:
        tally = {oid: [0, 0, 0] for oid in OPP_IDS}
        for g in st.games:
            if not g.truncated:
                tally[g.black if g.learner_side else g.white][("win", "loss", "draw").index(g.learner_result)] += 1
        assert tally == st.opponent_results
        assert len([g for g in st.games if not g.truncated]) == st.terminated
        assert len([g for g in st.games if g.truncated]) == st.truncated
    for g in got:
        assert g.is_standard_start and 1 <= len(g.actions) <= MAX_PLY
        _replays_on_the_oracle(g, MAX_PLY)
    # the games still in progress: the host log's peek, named by the players seated now
    live = base["live"]
    rows = host.peek(side=base["side"], opp=base["opp"], ids=ids, ply_counter=TOTAL)
    assert [_key(g) for g in live] == [_key(g) for g in games_from_records(rows)]
    assert len(live) == N and all(not g.finished and g.end_ply == TOTAL and not g.carried for g in live)
    assert sum(len(g.actions) == THIRD for g in live) >= N // 2
    for g in live:
        assert g.actions.tolist() == [int(r["actions"][g.env]) for r in records[TOTAL - len(g.actions):]]
    assert [_key(g) for g in base["some"]] == [_key(live[e]) for e in (5, 5, 63)]
    for g in live[:8]:
        _replays_on_the_oracle(g, MAX_PLY)


def test_a_graph_gives_the_same_games_and_rows():
    base = _base()
    _, stats, _, cols = _epochs(256, graph=True)
    assert [[_key(g) for g in st.games] for st in stats] == [[_key(g) for g in st.games] for st in base["stats"]]
    assert all(st.games_dropped == 0 for st in stats)
    for k, v in base["cols"].items():
        assert _same_bits(cols[k], v), k


@pytest.mark.parametrize("game_log", [None, 0], ids=["no-keyword", "game_log0"])
def test_the_log_does_not_disturb_the_epoch(game_log):
    base = _base()
    roll, stats, _, cols = _epochs(game_log)
    assert roll.game_log is None
    for k, v in base["cols"].items():
        assert _same_bits(cols[k], v), k
    for st, ref in zip(stats, base["stats"]):
        assert st.games == [] and st.games_dropped == 0
        a, b = dict(st.__dict__), dict(ref.__dict__)
        for d in (a, b):
            del d["games"], d["games_dropped"]
        assert a == b
    with pytest.raises(ValueError, match="game_log > 0"):
        roll.live_games()


@pytest.mark.parametrize("new_k", [3, 2], ids=["same-K", "other-K"])
def test_a_new_cohort_in_the_middle_of_a_run(new_k):
    ms = _models(K3 + 1)
    roll = _roll(256, record=True)
    ids_before = roll._ids.data_ptr()
    buf = KataGoRolloutBuffer(N, OBS, ACTION_SPACE, device=DEV)
    st1 = roll.collect(buf, 6)
    records = list(roll.record)
    new_ids = [71, 72, 73][:new_k]
    roll.set_opponents(list(reversed(ms[1:]))[:new_k], new_ids)
    assert (roll._ids.data_ptr() == ids_before) == (new_k == K3)
    assert roll._ids.cpu().tolist() == [LEARNER_ID, *new_ids]
    st2 = roll.collect(buf, 18)
    records += roll.record
    records[6] = dict(records[6], ids=np.asarray([LEARNER_ID, *new_ids], np.int32),
                      seat=(np.zeros((1, 4), np.int32), 1, N))
    host = game_log_host(records, num_envs=N, max_ply=MAX_PLY, capacity=1024, ids=np.asarray([LEARNER_ID, *OPP_IDS], np.int32))
    got = st1.games + st2.games
    assert [_key(g) for g in got] == [_key(g) for g in host.games()]
    assert st1.games_dropped == st2.games_dropped == 0 and len(got) >= 2 * N
    spanning = [g for g in got if g.end_ply - len(g.actions) + 1 < 6 <= g.end_ply]
    after = [g for g in got if g.end_ply - len(g.actions) + 1 >= 6]
    assert len(spanning) >= N // 2 and all(g.carried for g in spanning)
    assert len(after) >= N // 2 and not any(g.carried for g in after)
    for g in spanning + after:                                   # every game that ended under the new cohort
        assert (g.black if g.learner_side else g.white) in new_ids and LEARNER_ID in (g.black, g.white)
    assert set(st2.opponent_results) == set(new_ids)


def test_live_games_of_the_other_owners():
    roll = SelfPlayRollout(_models(1)[0], num_envs=5, max_ply=8, graph=False, sync_every=4, seed=1, game_log=64, record=True)
    roll.collect(KataGoRolloutBuffer(5, OBS, ACTION_SPACE, device=DEV), 11)
    live = roll.live_games()
    assert [g.env for g in live] == list(range(5)) and all(not g.finished and g.end_ply == 11 for g in live)
    assert all((g.black, g.white, g.learner_side) == (-1, -1, None) and 1 <= len(g.actions) <= 3 for g in live)
    for g in live:
        assert g.actions.tolist() == [int(r["actions"][g.env]) for r in roll.record[11 - len(g.actions):]]
    assert [_key(g) for g in roll.live_games([4, 0])] == [_key(live[4]), _key(live[0])]
    for g in live:
        _replays_on_the_oracle(g, 8)
    with pytest.raises(ValueError, match=r"envs must lie in \[0, 5\)"):
        roll.live_games([5])
    with pytest.raises(ValueError, match="game_log > 0"):
        SelfPlayRollout(_models(1)[0], num_envs=5, max_ply=8, graph=False, sync_every=4, seed=1).live_games()
    group = SEResNetGroup(_models(2))
    arena = MatchArena(group, 8, 4, 6, sync_every=2, graph=False, seed=11, game_log=64)
    arena.run_round([(0, 1), (1, 0), (0, 1)], games_per_match=4)
    live = arena.live_games()
    assert [g.env for g in live] == list(range(8)) and all(not g.finished and g.learner_side is None for g in live)
    assert all(len(g.actions) <= 6 for g in live)
    for g in live:
        _replays_on_the_oracle(g, 6)
    with pytest.raises(ValueError, match="game_log > 0"):
        MatchArena(group, 8, 4, 6, sync_every=2, graph=False, seed=11).live_games()


def test_league_games_become_an_sl_dataset():
    base = _base()
    games = [g for st in base["stats"] for g in st.games]
    ds, meta = dataset_from_recorded_games(games, batch_envs=64, max_moves=MAX_PLY)
    total = sum(len(g.actions) for g in games)
    assert len(ds) == total == meta["num_positions"] and meta["num_games"] == len(games)
    assert meta["games_nonstandard_start"] == meta["games_cut_illegal"] == meta["games_cut_by_rules"] == 0
    got = ds.read_batch(np.arange(total))
    assert np.array_equal(got["policy_target"].cpu().numpy(), np.concatenate([g.actions.astype(np.int64) for g in games]))
    with pytest.raises(ValueError, match="in progress"):
        dataset_from_recorded_games(games[:2] + base["live"][:1], batch_envs=4, max_moves=MAX_PLY)
