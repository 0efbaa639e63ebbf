"""LeagueRollout on the GPU: ka_league_step against the host restatement of the reference's protocol (word for word, with
guard bands), whole epochs against the restatement of their own records, invariance under sync_every / graph capture,
log-probs and values against the samplers and the learner's own forward, refresh(), KataGoPPOAlgorithm.update on the
collected buffer, and the errors raised at the sync point.

Small models (2 blocks, 128 channels) with their own weights each and max_ply = 40, so that truncations and restarts
are plentiful within a short epoch."""
import gc
import math

import numpy as np
import pytest
import torch

from keisei_amd import _lib
from keisei_amd.shogi_gym import ACTION_SPACE, MASK_WORDS
from keisei_amd.training import LeagueRollout
from keisei_amd.training.katago_ppo import _FIELDS, KataGoPPOAlgorithm, KataGoPPOParams, KataGoRolloutBuffer
from keisei_amd.training.league_rollout import (_HDR, _BLOCKS, _DROPPED, _ROWS, _TRUNC, _league_host, cum_thresholds,
                                                draw_opponents, draw_sides)
from keisei_amd.training.model_group import SEResNetGroup
from keisei_amd.training.models.se_resnet import SEResNetModel, SEResNetParams
from keisei_amd.training.value_adapter import MultiHeadValueAdapter
from oracle import keisei_oracle as orc
from oracle import shogi as S

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPE = orc.NetShape(2, 128, 8, 64, 16, 128, 64)
MAX_PLY = 40
OBS = (50, 9, 9)
COLUMNS = ("observations", "actions", "log_probs", "values", "rewards", "dones", "terminated", "legal_masks",
           "value_categories", "score_targets", "env_ids", "next_value_override")
_MODELS = []


@pytest.fixture(autouse=True)
def _release_device_objects():
    """A rollout object owns captured graphs and pinned host buffers.  One that an exception's traceback keeps in a
    reference cycle (the error tests) is freed by the garbage collector at a time of its choosing, which may be inside a
    later test's graph capture, where releasing such objects is not allowed: collect here, with the device idle."""
    yield
    gc.collect()
    torch.cuda.synchronize()
    gc.collect()


def _models(n):
    while len(_MODELS) < n:
        m = SEResNetModel(SEResNetParams(**SHAPE.__dict__))
        m.load_state_dict(orc.init_like_state_dict(SHAPE, salt=31 * len(_MODELS) + 7), strict=True)
        _MODELS.append(m.to(DEV).eval())
    return _MODELS[:n]


def _stream():
    return _lib.stream_ptr(torch.device(DEV))


def _same(a, b, key=""):
    """bitwise equality of two tensors / arrays (NaN equals NaN)"""
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else np.asarray(b)
    assert a.shape == b.shape, (key, a.shape, b.shape)
    if a.dtype.kind == "f":
        assert np.array_equal(a.astype(np.float32).view(np.uint32) | (np.isnan(a) * np.uint32(0xFFFFFFFF)),
                              b.astype(np.float32).view(np.uint32) | (np.isnan(b) * np.uint32(0xFFFFFFFF))), key
    else:
        assert np.array_equal(a, b), key


def _same_columns(got: dict, want: dict, rows=None):
    for key in COLUMNS:
        g = got[key]
        if key == "next_value_override" and key not in want:               # a host buffer that never saw an override has no column
            assert bool(torch.isnan(g).all())
            continue
        _same(g if rows is None else g[:rows], want[key] if rows is None else want[key][:rows], key)


# ------------------------------------------------------------------ 1. the kernel against the host restatement
SENT_F, SENT_I, SENT_B, GUARD = -777.25, 0x5A5A5A5A, 0xA5, 3
SMALL_OBS, SMALL_A, SMALL_MAX_PLY = (2, 3, 3), 40, 6


def _facts(E, T, seed, obs_shape):
    """T plies of env facts, as tools/make_league_golden.py builds them: players alternate inside a game, a game ends by a
    random result or at SMALL_MAX_PLY plies, and the next game starts with player 0."""
    g = np.random.default_rng(seed)
    player, ply = np.zeros(E, np.uint8), np.zeros(E, np.int64)
    out = []
    for _ in range(T):
        masks = g.random((E, SMALL_A)) < 0.3
        actions = g.integers(0, SMALL_A, E)
        masks[np.arange(E), actions] = True
        ends = g.random(E) < 0.2
        result = g.choice(np.array([1.0, -1.0, 0.0], np.float32), E, p=[0.5, 0.25, 0.25])
        ply = ply + 1
        truncated = ~ends & (ply >= SMALL_MAX_PLY)
        done = ends | truncated
        nxt = np.where(done, 0, 1 - player).astype(np.uint8)
        out.append(dict(obs=g.random((E, *obs_shape)).astype(np.float32), legal_masks=masks, pre_players=player.copy(),
                        actions=actions.astype(np.int64), log_probs=(-g.random(E) * 3).astype(np.float32),
                        vlogits=g.standard_normal((E, 3)).astype(np.float32), score_lead=(g.standard_normal(E) * 2).astype(np.float32),
                        rewards=np.where(ends, result, 0).astype(np.float32), terminated=ends.copy(), truncated=truncated.copy(),
                        current_players=nxt.copy(), material=g.integers(-60, 61, E).astype(np.int32),
                        term_obs=g.random((E, *obs_shape)).astype(np.float32),
                        term_values=np.where(truncated, g.random(E) * 2 - 1, np.nan).astype(np.float32)))
        player, ply = nxt, np.where(done, 0, ply)
    return out


class _Rig:
    """Device buffers of ka_league_step with guard bands behind every column, the pending slots and the truncation slots."""

    def __init__(self, E, K, obs_shape, cap, seed, cum, side, opp, color, alpha, score_norm):
        self.E, self.K, self.cap, self.alpha, self.score_norm, self.color = E, K, cap, alpha, score_norm, color
        self.oe, self.words = int(np.prod(obs_shape)), (SMALL_A + 31) // 32
        f = lambda *s: torch.full(s, SENT_F, device=DEV)  # noqa: E731
        i = lambda *s, dt=torch.int32: torch.full(s, SENT_I if dt != torch.uint8 else SENT_B, dtype=dt, device=DEV)  # noqa: E731
        R = cap + GUARD
        self.cols = dict(observations=f(R, self.oe), legal_masks=i(R, self.words), actions=i(R, dt=torch.int64), log_probs=f(R),
                         values=f(R), rewards=f(R), dones=i(R, dt=torch.uint8), terminated=i(R, dt=torch.uint8),
                         value_categories=i(R, dt=torch.int64), score_targets=f(R), env_ids=i(R, dt=torch.int64),
                         next_value_override=f(R))
        self.desc = torch.tensor([*(self.cols[k].data_ptr() for k in (
            "observations", "legal_masks", "actions", "log_probs", "values", "rewards", "dones", "terminated",
            "value_categories", "score_targets", "env_ids", "next_value_override")), 0, cap], dtype=torch.int64, device=DEV)
        assert self.desc.numel() == _lib.query("ka_league_layout", 1)
        self.p_obs, self.p_bits = f(E + GUARD, self.oe), i(E + GUARD, self.words)
        self.pcols = _lib.query("ka_league_layout", 2)
        self.p_scal = i(self.pcols * E + GUARD)
        self.p_scal[:self.pcols * E] = 0
        self.t_obs, self.t_list = f(E + GUARD, self.oe), i(E + GUARD, _lib.query("ka_league_layout", 3))
        self.plan = i(E * _lib.query("ka_league_layout", 0) + GUARD)
        st = torch.zeros(_lib.query("ka_league_state_words", K), dtype=torch.int32)
        st[0:2].view(torch.int64)[0] = 1234
        st[10:12].view(torch.int64)[0] = seed
        self.state = st.to(DEV)
        self.side, self.opp = torch.from_numpy(side.copy()).to(DEV), torch.from_numpy(opp.copy()).to(DEV)
        self.games = torch.zeros(E, dtype=torch.int32, device=DEV)
        self.cum = torch.from_numpy(cum.view(np.int32).copy()).to(DEV)
        self.model_of = torch.full((E,), -7, dtype=torch.int32, device=DEV)
        self.stall = torch.zeros(E, dtype=torch.uint8, device=DEV)
        self.values = torch.zeros(E, device=DEV)

    def step(self, rec, flush=0, nlegal=None):
        E = self.E
        d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)  # noqa: E731
        if flush:
            args = [None] * 6 + [0.0] + [None] * 7 + [1.0] + [None] * 6 + [0, None, None, None]
        else:
            bits = torch.zeros(E, self.words, dtype=torch.int32, device=DEV)
            _lib.call("ka_pack_mask_bits", d(rec["legal_masks"]), bits, E, SMALL_A, _stream())
            self.keep = [d(rec[k]) for k in ("obs", "actions", "log_probs", "vlogits", "score_lead")]
            self.keep += [bits, torch.ones(E, dtype=torch.int32, device=DEV) if nlegal is None else d(nlegal)]
            self.keep += [d(rec[k]) for k in ("pre_players", "rewards", "terminated", "truncated", "current_players", "material", "term_obs")]
            o, a, lp, vl, sc, bits, nl, pre, rw, tm, tr, cur, mat, tob = self.keep
            args = [o, bits, a, lp, vl, sc if self.alpha else None, self.alpha, nl, pre, rw, tm, tr, cur, mat, self.score_norm, tob,
                    None, self.side, self.opp, self.games, self.cum, int(self.color), self.model_of, self.stall, self.values]
        _lib.call("ka_league_step", self.state, E, self.K, flush, *args, self.p_obs, self.p_bits, self.p_scal,
                  self.t_obs if not flush else None, self.t_list if not flush else None, self.desc, self.plan, self.oe,
                  self.words, _stream())
        torch.cuda.synchronize()

    def guards_intact(self, rows):
        for k, c in self.cols.items():
            tail = c[rows:]
            want = SENT_F if c.dtype == torch.float32 else (SENT_B if c.dtype == torch.uint8 else SENT_I)
            assert bool((tail == want).all()), f"column {k} written behind row {rows}"
        E = self.E
        assert bool((self.p_obs[E:] == SENT_F).all()) and bool((self.p_bits[E:] == SENT_I).all())
        assert bool((self.p_scal[self.pcols * E:] == SENT_I).all()) and bool((self.plan[-GUARD:] == SENT_I).all())
        assert bool((self.t_obs[E:] == SENT_F).all()) and bool((self.t_list[E:] == SENT_I).all())


def _scalar_values(vlogits, score, alpha):
    n = vlogits.shape[0]
    out = torch.empty(n, device=DEV)
    _lib.call("ka_scalar_value", torch.from_numpy(vlogits).to(DEV), torch.from_numpy(score).to(DEV) if alpha else None, alpha,
              out, n, _stream())
    return out.cpu().numpy()


def _run_kernel_case(E, K, *, T=26, color=True, alpha=0.25, obs_shape=SMALL_OBS, cap=None, every=1, seed=77):
    facts = _facts(E, T, 1000 * E + K, obs_shape)
    weights = None if K == 1 else [1.0, 2.0, 0.0, 1.5, 0.5][:K]
    cum = cum_thresholds(weights, K)
    envs = np.arange(E)
    side0 = draw_sides(seed, envs, np.zeros(E, np.int64)) if color else np.zeros(E, np.uint8)
    opp0 = draw_opponents(seed, envs, np.zeros(E, np.int64), cum)
    ids = [100 + 7 * k for k in range(K)]
    score_norm = 76.0
    for rec in facts:                                           # the values the kernel must compute: ka_scalar_value's arithmetic
        rec["all_values"] = _scalar_values(rec["vlogits"], rec["score_lead"], alpha)
    # host: values are the learner's where it moved (the restatement zeroes the rest itself)
    trace = []
    want, wstats = _league_host([dict(r, values=r["all_values"]) for r in facts], num_envs=E, obs_shape=obs_shape,
                                action_space=SMALL_A, opponent_ids=ids, seed=seed, cum=cum, color_randomization=color,
                                score_norm=score_norm, side=side0, opp=opp0, trace=trace)
    total = int(want["actions"].shape[0])
    rig = _Rig(E, K, obs_shape, total if cap is None else cap, seed, cum, side0, opp0, color, alpha, score_norm)
    side_before = side0
    last_sync = -1
    for t, (rec, tr) in enumerate(zip(facts, trace)):
        rig.step(rec)
        moved = rec["pre_players"] == side_before
        _same(rig.values, np.where(moved, rec["all_values"], 0).astype(np.float32), "values out")
        _same(rig.side, tr["side"], "side"); _same(rig.opp, tr["opp"], "opp"); _same(rig.games, tr["games"].astype(np.int32), "games")
        _same(rig.model_of, tr["model_of"], "model_of")
        ps = rig.p_scal[:rig.pcols * E].view(rig.pcols, E)
        _same(ps[5] != 0, tr["valid"], "pending valid")
        v, vd = tr["valid"], torch.from_numpy(tr["valid"]).to(DEV)
        _same(ps[3].view(torch.float32)[vd], tr["rewards"][v], "pending rewards")
        # the whole slot, where one is open, against the host PendingTransitions: observation, packed mask and scalars
        _same(rig.p_obs[:E][vd], tr["obs"][v].reshape(int(v.sum()), rig.oe), "pending obs")
        _same(rig.p_bits[:E][vd], tr["mask_bits"][v], "pending mask")
        _same(ps[0][vd].to(torch.int64), tr["actions"][v], "pending actions")
        _same(ps[1].view(torch.float32)[vd], tr["log_probs"][v], "pending log_probs")
        _same(ps[2].view(torch.float32)[vd], tr["values"][v], "pending values")
        _same(ps[4].view(torch.float32)[vd], tr["score_targets"][v], "pending score targets")
        side_before = tr["side"]
        if cap is None and ((t + 1) % every == 0 or t == T - 1):   # the host's part of the deferred override, as at a sync point
            st = rig.state.cpu().numpy()
            n = int(st[_TRUNC])
            tl = rig.t_list[:n].cpu().numpy()
            for j, (e, row, who) in enumerate(tl):
                ply = max(p for p in range(last_sync + 1, t + 1) if facts[p]["truncated"][e] and not facts[p]["terminated"][e])
                _same(rig.t_obs[j], facts[ply]["term_obs"][e].reshape(-1), "truncation slot")
                v = facts[ply]["term_values"][e]
                rig.cols["next_value_override"][row] = float(-v if (who & 1) != (who >> 1) else v)
            rig.state[_TRUNC:_TRUNC + 1].zero_()
            last_sync = t
    rig.step(None, flush=1)
    st = rig.state.cpu().numpy()
    rows = min(total, rig.cap)
    assert int(st[_ROWS]) == rows and int(st[_DROPPED]) == total - rows
    rig.guards_intact(rows)
    got = dict(rig.cols)
    got["observations"] = got["observations"].view(-1, *obs_shape)
    masks = torch.empty(rows + GUARD, SMALL_A, dtype=torch.bool, device=DEV)
    _lib.call("ka_unpack_mask_bits", got["legal_masks"], None, masks, rows + GUARD, SMALL_A, _stream())
    got["legal_masks"] = masks
    got["dones"], got["terminated"] = got["dones"].bool(), got["terminated"].bool()
    if cap is None:
        _same_columns({k: v[:rows] for k, v in got.items()}, want)
        assert int(st[_BLOCKS]) == want["size"]
        for k in ("wins", "losses", "draws", "black_wins", "white_wins", "terminated", "truncated"):
            assert int(st[{"wins": 14, "losses": 15, "draws": 16, "black_wins": 17, "white_wins": 18, "terminated": 19,
                           "truncated": 20}[k]]) == wstats[k], k
        res = {ids[k]: [int(v) for v in st[_HDR + 3 * k:_HDR + 3 * k + 3]] for k in range(K)}
        assert res == wstats["opponent_results"]
        assert not st[[21, 22, 23, 25, 26]].any()                 # no guard, conflict or zero-legal flag
        assert 0 < float(st[24:25].view(np.float32)[0]) <= 60 / 76.0 + 1e-6       # word 24: bits of max |score target|
    else:
        for key in COLUMNS[:-1]:
            _same(got[key][:rows], want[key][:rows], key)
    return wstats, want


@pytest.mark.parametrize("E", [3, 64, 300, 512])
@pytest.mark.parametrize("K", [1, 5])
def test_league_step_equals_the_host_restatement(E, K):
    wstats, want = _run_kernel_case(E, K, every=1 if E < 300 else 4)
    if E >= 64:                                                   # every branch occurred
        assert wstats["truncated"] and wstats["draws"] and wstats["truncation_overrides"]
        assert bool((want["dones"] & want["terminated"]).any()) and bool((~want["dones"]).any())


def test_league_step_odd_row_length_no_blend_fixed_colour():
    _run_kernel_case(70, 3, obs_shape=(3, 3, 3), alpha=0.0, color=False)


def test_league_step_writes_nothing_past_the_reserved_rows():
    _run_kernel_case(64, 2, cap=37)
    _run_kernel_case(300, 1, cap=5)


def test_league_step_raises_the_input_guards_and_the_zero_legal_latches():
    """the twin of the self-play step's test, on the league's three ways to a row.  Fixed colour, so the learner is player 0.
    Ply 0, every env a learner move: env 3 terminates with a NaN reward, a label outside {-1, 0, 1, 2} on its immediate row;
    env 0 has no legal action (a learner row).  Ply 1, the opponent's reply in envs 0, 1, 2, 4 settles their rows; env 2 has
    no legal action (an opponent row); env 3, a new game, opens a slot with a material beyond 3.5 score_norm, and the flush
    settles it: the peak word shows that the flush reaches the same commit."""
    E, norm = 5, 76.0
    p0, p1 = _facts(E, 2, 11, SMALL_OBS)
    calm = dict(rewards=np.zeros(E, np.float32), terminated=np.zeros(E, bool), truncated=np.zeros(E, bool))
    p0.update({k: v.copy() for k, v in calm.items()}, pre_players=np.zeros(E, np.uint8),
              current_players=np.array([1, 1, 1, 0, 1], np.uint8))
    p0["terminated"][3], p0["rewards"][3] = True, np.nan
    p1.update({k: v.copy() for k, v in calm.items()}, pre_players=p0["current_players"].copy(),
              current_players=np.array([0, 0, 0, 1, 0], np.uint8))
    p1["material"][3] = 400
    rig = _Rig(E, 1, SMALL_OBS, 8, 77, cum_thresholds(None, 1), np.zeros(E, np.uint8), np.zeros(E, np.int32), False, 0.25, norm)
    peak = lambda st: float(st[24:25].view(np.float32)[0])  # noqa: E731
    score = lambda m: np.float32(m) / np.float32(norm)  # noqa: E731

    rig.step(p0, nlegal=np.array([0, 1, 1, 1, 1], np.int32))
    st = rig.state.cpu().numpy()
    assert int(st[_ROWS]) == 1 and int(rig.cols["value_categories"][0]) == 3 and int(rig.cols["env_ids"][0]) == 3
    assert st[21] == 0 and st[22] == 1 and st[23] == 0 and peak(st) == abs(score(p0["material"][3]))
    assert st[26] == 1 and rig.stall.tolist() == [1, 0, 0, 0, 0]

    rig.step(p1, nlegal=np.array([1, 1, 0, 1, 1], np.int32))
    st = rig.state.cpu().numpy()
    assert int(st[_ROWS]) == 5 and rig.cols["env_ids"][1:5].tolist() == [0, 1, 2, 4]
    assert st[21] == 0 and st[22] == 1 and st[23] == 0 and peak(st) == score(np.abs(p0["material"]).max())
    assert st[25] == 0 and st[26] == 3 and rig.stall.tolist() == [1, 0, 2, 0, 0]

    rig.step(None, flush=1)
    st = rig.state.cpu().numpy()
    assert int(st[_ROWS]) == 6 and int(rig.cols["env_ids"][5]) == 3 and int(rig.cols["value_categories"][5]) == -1
    assert st[21] == 0 and st[22] == 1 and st[23] == 0 and peak(st) == score(400)
    assert st[25] == 0 and st[26] == 3 and rig.stall.tolist() == [1, 0, 2, 0, 0]      # latches: the flush clears neither
    rig.guards_intact(6)


# ------------------------------------------------------------------ whole epochs
def _roll(N, *, K=3, color=True, alpha=0.25, **kw):
    ms = _models(K + 1)
    adapter = MultiHeadValueAdapter(score_blend_alpha=alpha) if alpha is not None else None
    kw.setdefault("seed", 4242)
    return LeagueRollout(ms[0], ms[1:], [10 * k + 3 for k in range(K)], num_envs=N, max_ply=MAX_PLY, value_adapter=adapter,
                         color_randomization=color, opponent_weights=[1.0, 2.0, 1.0, 1.0, 1.0][:K], **kw)


def _buffer(N):
    return KataGoRolloutBuffer(N, OBS, ACTION_SPACE, device=DEV)


def _term_values(roll, rec):
    """the learner's value of the recorded terminal observations, by a grouped forward of its own (model 0 on every row)"""
    N = roll.num_envs
    out = np.full(N, np.nan, np.float32)
    envs = rec["terminal_envs"]
    if len(envs):
        obs = rec["terminal_obs"].to(DEV)
        o = roll.group.forward(obs, torch.zeros(len(envs), dtype=torch.int32, device=DEV))
        v = torch.empty(len(envs), device=DEV)
        _lib.call("ka_scalar_value", o.value_logits.contiguous(), o.score_lead.reshape(-1).contiguous() if roll.alpha else None,
                  roll.alpha, v, len(envs), _stream())
        out[envs] = v.cpu().numpy()
    return out


def _host_of(roll, records, side0, opp0, games0):
    recs = [dict(r, term_values=_term_values(roll, r)) for r in records]
    return _league_host(recs, num_envs=roll.num_envs, obs_shape=OBS, action_space=ACTION_SPACE, opponent_ids=roll.opponent_ids,
                        seed=roll._draw_seed, cum=roll._cum_host, color_randomization=roll.color_randomization,
                        score_norm=roll.score_norm, side=side0, opp=opp0, games=games0)


def _stats_dict(stats):
    return {k: getattr(stats, k) for k in ("plies", "rows", "adds", "wins", "losses", "draws", "black_wins", "white_wins",
                                           "terminated", "truncated", "opponent_results", "truncation_overrides")}


@pytest.mark.parametrize("N,color", [(64, True), (64, False), (512, True)])
def test_recorded_epoch_equals_its_host_restatement(N, color):
    roll = _roll(N, color=color, graph=False, record=True, sync_every=8)
    buf = _buffer(N)
    stats = roll.collect(buf, 44)
    records = roll.record
    side0, opp0 = records[0]["side"], records[0]["opp"]
    want, wstats = _host_of(roll, records, side0, opp0, np.zeros(N, np.int64))
    got = buf.flatten()
    _same_columns(got, want)
    assert buf.size == want["size"] and _stats_dict(stats) == wstats
    assert stats.truncated > 0 and stats.truncation_overrides > 0 and bool(torch.isfinite(got["next_value_override"]).any())
    assert stats.host_syncs <= math.ceil(44 / 8) + 2
    if color:
        assert {0, 1} <= set(np.unique(np.stack([r["side"] for r in records])))
    # the recorded seating is the restated one: learner where the side is to move, else the env's opponent + 1
    for r in records:
        assert np.array_equal(r["model_of"], np.where(r["pre_players"] == r["side"], 0, r["opp"] + 1))


# ------------------------------------------------------------------ invariance
def _epoch(N, steps, *, color, calls=1, **kw):
    roll = _roll(N, color=color, **kw)
    buf = _buffer(N)
    parts = steps if isinstance(steps, (list, tuple)) else [steps // calls] * calls
    stats = [roll.collect(buf, n) for n in parts]
    cols = {k: v.clone() for k, v in buf.flatten().items()}
    return roll, cols, stats, buf.size


def test_one_seed_gives_one_epoch_whatever_the_schedule():
    N, steps = 64, 64
    ref_roll, ref, ref_stats, ref_size = _epoch(N, steps, color=True, graph=False, record=True, sync_every=2)
    records = ref_roll.record
    sides = np.stack([r["side"] for r in records])
    moved = np.stack([r["pre_players"] for r in records]) == sides
    done = np.stack([r["terminated"] | r["truncated"] for r in records])
    trunc = np.stack([r["truncated"] & ~r["terminated"] for r in records])
    assert trunc.any(), "no truncation in the epoch"
    assert (moved & done).any(), "no immediate settle in the epoch"
    assert (sides == 0).any() and (sides == 1).any(), "one colour only"
    assert ref_stats[0].truncation_overrides > 0
    for kw in (dict(graph=True, sync_every=2), dict(graph=False, sync_every=8), dict(graph=True, sync_every=8),
               dict(graph=True, sync_every=32), dict(graph=False, sync_every=32)):
        _, cols, stats, size = _epoch(N, steps, color=True, **kw)
        _same_columns(cols, ref)
        assert size == ref_size and _stats_dict(stats[0]) == _stats_dict(ref_stats[0]), kw


@pytest.mark.parametrize("parts", [(32, 32), (31, 33)], ids=["32+32", "31+33"])
def test_one_collect_of_64_against_two_of_32(parts):
    """With every env starting on the learner's move and no game ending early, the opponent has just replied after 32 plies:
    the first call's flush finds nothing open and the two buffers are identical in full.  After 31 plies every env holds an
    open transition, and the flush closes all of them early.  In general the games are the same; the rows differ only where the first call's flush at its end (katago_loop.py:1537-1563, which
    collect() owes every call) closes a transition early: such a row leaves with done = 0, without the opponent's reply
    in its reward, without a label and without a truncation override.  So: per env, the sequence of learner moves
    (observation, action, log-prob, value, score target) is identical; every row outside the first call's flush block is
    identical in every column; tallies and per-opponent results add up; and the overrides of the single call exceed the
    two calls' by exactly the flushed rows whose game the opponent's reply then truncated.  Colour randomisation is off,
    because the reference re-draws all sides at the start of every epoch (:1134-1137), which two calls do twice."""
    N = 64
    _, one, s1, _ = _epoch(N, 64, color=False, graph=True, sync_every=8)
    _, two, s2, _ = _epoch(N, list(parts), color=False, graph=True, sync_every=8)
    assert one["actions"].shape == two["actions"].shape
    o1, o2 = torch.argsort(one["env_ids"], stable=True), torch.argsort(two["env_ids"], stable=True)
    for key in ("env_ids", "observations", "actions", "log_probs", "values", "score_targets", "legal_masks"):
        _same(one[key][o1], two[key][o2], key)
    assert s2[0].flushed <= N and s1[0].flushed == s2[1].flushed
    assert s2[0].flushed > 0 if parts[0] % 2 else True, "an odd first call must leave open transitions to its flush"
    flush = (o2 >= s2[0].rows - s2[0].flushed) & (o2 < s2[0].rows)          # the rows the first call's flush closed
    assert int(flush.sum()) == s2[0].flushed
    for key in ("rewards", "dones", "terminated", "value_categories", "next_value_override"):
        _same(one[key][o1][~flush], two[key][o2][~flush], key)
    assert bool((~two["dones"][o2][flush]).all()) and bool((two["value_categories"][o2][flush] == -1).all())
    assert bool(torch.isnan(two["next_value_override"][o2][flush]).all())
    late = int(torch.isfinite(one["next_value_override"][o1][flush]).sum())
    assert s1[0].truncation_overrides == s2[0].truncation_overrides + s2[1].truncation_overrides + late
    for k in ("wins", "losses", "draws", "black_wins", "white_wins", "terminated", "truncated"):
        assert getattr(s1[0], k) == getattr(s2[0], k) + getattr(s2[1], k), k
    for oid, res in s1[0].opponent_results.items():
        assert res == [a + b for a, b in zip(s2[0].opponent_results[oid], s2[1].opponent_results[oid])], oid
    assert s1[0].truncated > 0


def test_set_opponents_seats_a_new_cohort_under_graph_and_eager():
    """collect, a cohort of another size, collect again: the graph form (graphs dropped and captured again, the state's
    header kept, opponents drawn anew from the games finished so far) against the eager form, and a learner refresh in
    between, which the captured graph must see."""
    N = 64
    ms = _models(5)
    out = []
    for graph in (True, False):
        roll = _roll(N, K=3, color=True, graph=graph, sync_every=8)
        buf = _buffer(N)
        first = roll.collect(buf, 48)
        roll.refresh()
        roll.set_opponents([ms[4], ms[2]], [77, 23], [1.0, 3.0])
        assert len(roll.group) == 3 and roll.opponent_ids == [77, 23] and not roll._graphs
        opp = roll._opp.cpu().numpy()
        games = roll._games.cpu().numpy()
        assert np.array_equal(opp, draw_opponents(roll._draw_seed, np.arange(N), games, cum_thresholds([1.0, 3.0], 2)))
        assert games.any() and set(np.unique(opp)) == {0, 1}
        second = roll.collect(buf, 40)
        assert set(second.opponent_results) == {77, 23} and second.rows > 0 and (not graph or roll._graphs)
        assert sum(sum(r) for r in second.opponent_results.values()) == second.terminated and second.truncated > 0
        out.append(({k: v.clone() for k, v in buf.flatten().items()}, _stats_dict(first), _stats_dict(second), buf.size))
    _same_columns(out[0][0], out[1][0])
    assert out[0][1:] == out[1][1:]


# ------------------------------------------------------------------ log-probs and values
def test_learner_rows_carry_the_samplers_log_probs_and_values(monkeypatch):
    N, alpha = 64, 0.25
    roll = _roll(N, color=True, alpha=alpha, graph=False, record=True, sync_every=4)
    buf = _buffer(N)
    roll.collect(buf, 12)
    learner = roll.learner
    for rec in roll.record[::3]:
        obs, bits = rec["obs"].to(DEV), rec["mask_bits"].to(DEV)
        mo = torch.from_numpy(rec["model_of"]).to(DEV)
        act, lp = roll.group.select_actions(obs, bits, mo, seed=rec["seed"])
        _same(act, rec["actions"], "actions"); _same(lp, rec["log_probs"], "log_probs")
        out = roll.group.forward(obs, mo)
        a2, l2, v2 = (torch.empty(N, dtype=torch.int64, device=DEV), torch.empty(N, device=DEV), torch.empty(N, device=DEV))
        nl, fl = torch.empty(N, dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
        _lib.call("ka_policy_sample", out.policy_logits.reshape(N, -1), 0, bits, MASK_WORDS, rec["seed"], out.value_logits,
                  out.score_lead.reshape(N).contiguous(), alpha, a2, l2, v2, nl, fl, N, ACTION_SPACE, _stream())
        rows = torch.from_numpy(rec["model_of"] == 0).to(DEV)
        assert bool(rows.any())
        _same(v2[rows], rec["values"][rows.cpu().numpy()], "values")
        assert not rec["values"][~rows.cpu().numpy()].any()
        # the learner module's own eval forward (bf16, per-layer path): the bound of tests/test_hip_model_group.py on the
        # logits, 0.02 max|logit| + 1e-3 =: eps; a log-prob moves by at most 2 eps, P(W) - P(L) by at most 2 eps_value
        monkeypatch.setenv("KA_EVAL_GRAPH", "0")
        with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
            own = learner(obs[rows].contiguous())
        pol = own.policy_logits.float().reshape(int(rows.sum()), -1)
        eps = 0.02 * float(pol.abs().max()) + 1e-3
        assert float((out.policy_logits.reshape(N, -1)[rows] - pol).abs().max()) <= eps
        masks = torch.empty(N, ACTION_SPACE, dtype=torch.bool, device=DEV)
        _lib.call("ka_unpack_mask_bits", bits, None, masks, N, ACTION_SPACE, _stream())
        ref_lp = torch.log_softmax(pol.masked_fill(~masks[rows], float("-inf")), dim=-1).gather(1, act[rows].unsqueeze(1)).squeeze(1)
        assert float((ref_lp - lp[rows]).abs().max()) <= 2 * eps
        vl = own.value_logits.float()
        eps_v = 0.02 * float(vl.abs().max()) + 1e-3
        eps_s = 0.02 * float(own.score_lead.float().abs().max()) + 1e-3
        ref_v = roll.value_adapter.scalar_value_blended(vl, own.score_lead.float())
        assert float((ref_v.reshape(-1) - v2[rows]).abs().max()) <= (1 - alpha) * 2 * eps_v + alpha * eps_s


# ------------------------------------------------------------------ refresh
def test_refresh_brings_in_place_weight_edits_into_the_ply():
    N = 16
    ms = []
    for k in range(2):
        m = SEResNetModel(SEResNetParams(**SHAPE.__dict__))
        m.load_state_dict(orc.init_like_state_dict(SHAPE, salt=900 + k), strict=True)
        ms.append(m.to(DEV).eval())
    roll = LeagueRollout(ms[0], ms[1:], [5], num_envs=N, max_ply=MAX_PLY, graph=False, sync_every=2, seed=1)

    def learner_logits():
        roll.reset()
        roll._ply()
        rows = (roll.env._players[roll.env._cur ^ 1] == roll._side)          # the learner moved first in every env (side 0)
        assert bool(rows.all())
        return roll._ws["logits"].clone()

    before = learner_logits()
    with torch.no_grad():
        ms[0].policy_conv2.bias.add_(0.5)
    stale = learner_logits()
    assert torch.equal(before, stale)                              # the group still holds the old snapshot
    roll.refresh()
    fresh = learner_logits()
    assert float((fresh - before).abs().max()) > 0.25


# ------------------------------------------------------------------ update
def test_ppo_update_runs_on_the_collected_buffer():
    N = 64
    roll = _roll(N, color=True, graph=False, record=True, sync_every=8)
    buf = _buffer(N)
    stats = roll.collect(buf, 44)
    records = roll.record
    want, _ = _host_of(roll, records, records[0]["side"], records[0]["opp"], np.zeros(N, np.int64))
    nv = roll.bootstrap_values()
    # bootstrap: the learner's value of the observation now, negated where the opponent is to move
    env = roll.env
    v = torch.from_numpy(_term_values(roll, dict(terminal_envs=np.arange(N), terminal_obs=env.current().observations.cpu()))).to(DEV)
    _same(nv, torch.where(env._players[env._cur] != roll._side, -v, v), "bootstrap values")
    ppo = KataGoPPOAlgorithm(KataGoPPOParams(batch_size=256, epochs_per_batch=1), roll.learner)
    data = buf.flatten_packed()
    adv = ppo._advantages(data, buf, nv, torch.device(DEV))
    host = KataGoRolloutBuffer(N, OBS, ACTION_SPACE)
    host._step_count = want["size"]
    hdata = {k: v for k, v in want.items() if k != "size"}
    adv_host = ppo._advantages(hdata, host, nv, torch.device(DEV))            # host columns, the same ka_gae scan
    assert adv.shape == adv_host.shape and stats.rows == adv.numel()
    assert torch.equal(adv.cpu(), adv_host.cpu())
    metrics = ppo.update(buf, nv, value_adapter=roll.value_adapter)
    assert metrics and all(math.isfinite(float(x)) for x in metrics.values()), metrics
    assert buf.size == 0
    roll.refresh()
    stats2 = roll.collect(buf, 8)                                  # the next epoch goes on from the games in progress
    assert stats2.rows > 0 and buf.size == stats2.adds


# ------------------------------------------------------------------ errors
def test_zero_legal_row_is_raised_at_the_sync_with_the_env_named():
    ms = _models(2)
    roll = LeagueRollout(ms[0], ms[1:], [1], num_envs=4, max_ply=MAX_PLY, graph=False, sync_every=2, seed=3)
    b, h = S.empty_board()                                        # game.rs:1061-1124: Black to move has no legal move
    b[S.sq(0, 0)] = S.KING; b[S.sq(2, 1)] = S.KING | S.WHITE
    b[S.sq(0, 1)] = b[S.sq(1, 0)] = b[S.sq(1, 1)] = S.PAWN | S.WHITE; b[S.sq(0, 5)] = S.ROOK | S.WHITE
    roll.env.set_state(2, b, h, 0)
    with pytest.raises(RuntimeError, match=r"Learner envs \[2\] have zero legal actions"):
        roll.collect(_buffer(4), 2)


def test_nan_weights_in_an_opponent_are_raised_at_the_sync():
    ms = []
    for k in range(2):
        m = SEResNetModel(SEResNetParams(**SHAPE.__dict__))
        m.load_state_dict(orc.init_like_state_dict(SHAPE, salt=700 + k), strict=True)
        ms.append(m.to(DEV).eval())
    with torch.no_grad():
        ms[1].policy_conv2.bias.fill_(float("nan"))
    roll = LeagueRollout(ms[0], ms[1:], [1], num_envs=8, max_ply=MAX_PLY, graph=False, sync_every=2, seed=3)
    with pytest.raises(RuntimeError, match="NaN in raw policy logits"):
        roll.collect(_buffer(8), 4)


def test_argument_errors_on_the_device():
    ms = _models(2)
    with pytest.raises(ValueError, match="must not exceed max_ply"):
        LeagueRollout(ms[0], ms[1:], [1], num_envs=8, max_ply=16, sync_every=32)
    with pytest.raises(ValueError, match="even sync_every"):
        LeagueRollout(ms[0], ms[1:], [1], num_envs=8, max_ply=MAX_PLY, sync_every=5, graph=True)
    wide = SEResNetModel(SEResNetParams(**orc.NetShape(2, 256).__dict__)).to(DEV).eval()
    with pytest.raises(ValueError, match="split_merge_step"):
        LeagueRollout(ms[0], [ms[1], wide], [1, 2], num_envs=8, max_ply=MAX_PLY, sync_every=4)
    roll = LeagueRollout(ms[0], ms[1:], [1], num_envs=8, max_ply=MAX_PLY, sync_every=4, graph=False)
    with pytest.raises(ValueError, match="steps must be positive"):
        roll.collect(_buffer(8), 0)
    with pytest.raises(ValueError, match="buffer holds"):
        roll.collect(KataGoRolloutBuffer(8, (46, 9, 9), ACTION_SPACE, device=DEV), 4)


def test_host_syncs_stay_within_the_bound_and_graphs_survive_a_growing_buffer():
    N = 64
    roll = _roll(N, color=True, graph=True, sync_every=8)
    buf = _buffer(N)
    buf._ensure_capacity = _tight(buf)                             # grow at every chunk: the descriptor must follow
    for steps in (44, 8, 13, 16):
        before = buf._write_offset
        stats = roll.collect(buf, steps)
        assert stats.host_syncs <= math.ceil(steps / 8) + 2
        assert buf._write_offset - before == stats.rows and stats.plies == steps
    cols = buf.flatten()
    assert bool(((cols["env_ids"] >= 0) & (cols["env_ids"] < N)).all())
    assert bool((cols["actions"] >= 0).all()) and bool((cols["actions"] < ACTION_SPACE).all())
    same_roll = _roll(N, color=True, graph=False, sync_every=8)
    buf2 = _buffer(N)
    for steps in (44, 8, 13, 16):
        same_roll.collect(buf2, steps)
    _same_columns(cols, buf2.flatten())
    del buf._ensure_capacity                                        # (the closure and the buffer name each other)


def _tight(buf):
    """an _ensure_capacity that allocates exactly what is asked, so that every reserve() moves the columns"""
    def ensure(n):
        need = buf._write_offset + n
        if need <= buf._alloc_samples:
            return
        keys = list(_FIELDS) + ["env_ids", "next_value_override"]
        grown = {k: buf._fresh(k, need) for k in keys}
        for k, t in grown.items():
            if k in buf._storage and buf._write_offset:
                t[:buf._write_offset] = buf._storage[k][:buf._write_offset]
        buf._storage, buf._alloc_samples = grown, need
    return ensure
