"""SelfPlayRollout on the GPU: ka_selfplay_step against the host restatement of the reference's no-opponent branch (word
for word, with guard bands), whole epochs against the restatement of their own records, invariance under sync_every /
graph capture / the split into collect calls, log-probs and values against the sampler, refresh(),
KataGoPPOAlgorithm.update on the collected buffer, and the errors raised at the sync point.

Small models (2 blocks, 128 channels) and a short max_ply, so that truncations and restarts are plentiful within a short
epoch."""
import gc
import math

import numpy as np
import pytest
import torch

from keisei_amd import _lib
from keisei_amd.shogi_gym import ACTION_SPACE, MASK_WORDS
from keisei_amd.training import SelfPlayRollout
from keisei_amd.training.katago_ppo import _FIELDS, KataGoPPOAlgorithm, KataGoPPOParams, KataGoRolloutBuffer
from keisei_amd.training.selfplay_rollout import _DROPPED, _ROWS, _TRUNC, _TRUNC_DROPPED, _selfplay_host
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
           "value_categories", "score_targets", "next_value_override")
TALLY_WORDS = {"wins": 14, "losses": 15, "draws": 16, "black_wins": 17, "white_wins": 18, "terminated": 19, "truncated": 20}
_MODELS = {}


@pytest.fixture(autouse=True)
def _release_device_objects():
    """A rollout object owns captured graphs and pinned host buffers.  One that an exception's traceback keeps in a
    reference cycle (the error tests) is freed by the garbage collector at a time of its choosing, which may be inside a
    later test's graph capture, where releasing such objects is not allowed: collect here, with the device idle."""
    yield
    gc.collect()
    torch.cuda.synchronize()
    gc.collect()


def _fresh_model(salt):
    m = SEResNetModel(SEResNetParams(**SHAPE.__dict__))
    m.load_state_dict(orc.init_like_state_dict(SHAPE, salt=salt), strict=True)
    return m.to(DEV).eval()


def _model(salt=7):
    if salt not in _MODELS:
        _MODELS[salt] = _fresh_model(salt)
    return _MODELS[salt]


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
    assert "env_ids" not in got and "env_ids" not in want
    for key in COLUMNS:
        g = got[key]
        if key == "next_value_override" and key not in want:               # a host buffer that never saw an override has no column
            assert bool(torch.isnan(g if rows is None else g[:rows]).all())
            continue
        _same(g if rows is None else g[:rows], want[key] if rows is None else want[key][:rows], key)


# ------------------------------------------------------------------ 1. the kernel against the host restatement
SENT_F, SENT_I, SENT_B, GUARD = -777.25, 0x5A5A5A5A, 0xA5, 3
SMALL_OBS, SMALL_A, SMALL_MAX_PLY = (2, 3, 3), 40, 6


def _facts(E, T, seed, obs_shape):
    """T plies of env facts, as tools/make_selfplay_golden.py builds them: every env begins somewhere inside a game, players
    alternate inside a game, a game ends by a random result or at SMALL_MAX_PLY plies (both flags where the last ply decides
    it), and the next game starts with player 0."""
    g = np.random.default_rng(seed)
    ply = g.integers(0, SMALL_MAX_PLY, E)
    player = (ply & 1).astype(np.uint8)
    out = []
    for _ in range(T):
        masks = g.random((E, SMALL_A)) < 0.3
        actions = g.integers(0, SMALL_A, E)
        masks[np.arange(E), actions] = True
        ends = g.random(E) < 0.2
        result = g.choice(np.array([1.0, -1.0, 0.0], np.float32), E, p=[0.5, 0.25, 0.25])
        ply = ply + 1
        truncated = ply >= SMALL_MAX_PLY
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


def _reaches_every_branch(facts):
    """the branches of the fixture's list (tests/test_selfplay_rollout_cpu.py), on a stream of facts"""
    st = lambda k: np.stack([f[k] for f in facts])  # noqa: E731
    tm, tr, r, pre = st("terminated"), st("truncated"), st("rewards"), st("pre_players")
    done, trunc = tm | tr, tr & ~tm
    return all(bool(x) for x in (
        (tm & (r > 0) & (pre == 0)).any(), (tm & (r > 0) & (pre == 1)).any(), (tm & (r < 0)).any(), (tm & (r == 0)).any(),
        trunc.any(), (done[1:] & done[:-1]).any(), trunc[0].any(), trunc[-1].any(), (tm[:-1] & ~done[1:]).any()))


def _facts_reaching_every_branch(E, T, obs_shape):
    for seed in range(1000 * E, 1000 * E + 500):                 # (three envs need a few tries, 64 and more none)
        facts = _facts(E, T, seed, obs_shape)
        if _reaches_every_branch(facts):
            return facts
    raise AssertionError(f"no stream of {E} envs reaches every branch")


class _Rig:
    """Device buffers of ka_selfplay_step with guard bands behind every column, the truncation slots and the plan."""

    def __init__(self, E, obs_shape, cap, alpha, score_norm):
        self.E, self.cap, self.alpha, self.score_norm = E, cap, alpha, score_norm
        self.oe, self.words = int(np.prod(obs_shape)), (SMALL_A + 31) // 32
        f = lambda *s: torch.full(s, SENT_F, device=DEV)  # noqa: E731
        i = lambda *s, dt=torch.int32: torch.full(s, SENT_I if dt != torch.uint8 else SENT_B, dtype=dt, device=DEV)  # noqa: E731
        R = cap + GUARD
        self.cols = dict(observations=f(R, self.oe), legal_masks=i(R, self.words), actions=i(R, dt=torch.int64), log_probs=f(R),
                         values=f(R), rewards=f(R), dones=i(R, dt=torch.uint8), terminated=i(R, dt=torch.uint8),
                         value_categories=i(R, dt=torch.int64), score_targets=f(R), env_ids=i(R, dt=torch.int64),
                         next_value_override=f(R))
        # (the descriptor names an env_ids column, which the kernel must leave alone: all of it is guard band)
        self.desc = torch.tensor([*(self.cols[k].data_ptr() for k in (
            "observations", "legal_masks", "actions", "log_probs", "values", "rewards", "dones", "terminated",
            "value_categories", "score_targets", "env_ids", "next_value_override")), 0, cap], dtype=torch.int64, device=DEV)
        assert self.desc.numel() == _lib.query("ka_selfplay_layout", 1)
        self.tw, self.pw = _lib.query("ka_selfplay_layout", 2), _lib.query("ka_selfplay_layout", 0)
        self.t_obs, self.t_list = f(E + GUARD, self.oe), i(E + GUARD, self.tw)
        self.plan = i(E * self.pw + GUARD)
        st = torch.zeros(_lib.query("ka_selfplay_state_words"), dtype=torch.int32)
        st[0:2].view(torch.int64)[0] = 1234
        self.state = st.to(DEV)
        self.stall = torch.zeros(E + GUARD, dtype=torch.uint8, device=DEV)
        self.values = f(E + GUARD)

    def step(self, rec, nlegal=None):
        E = self.E
        d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)  # noqa: E731
        bits = torch.zeros(E, self.words, dtype=torch.int32, device=DEV)
        _lib.call("ka_pack_mask_bits", d(rec["legal_masks"]), bits, E, SMALL_A, _stream())
        o, a, lp, vl, sc = (d(rec[k]) for k in ("obs", "actions", "log_probs", "vlogits", "score_lead"))
        nl = torch.ones(E, dtype=torch.int32, device=DEV) if nlegal is None else d(nlegal)
        pre, rw, tm, tr, mat, tob = (d(rec[k]) for k in ("pre_players", "rewards", "terminated", "truncated", "material", "term_obs"))
        _lib.call("ka_selfplay_step", self.state, E, o, bits, a, lp, vl, sc if self.alpha else None, self.alpha, nl, pre, rw, tm,
                  tr, mat, self.score_norm, tob, None, self.stall, self.values, self.t_obs, self.t_list, self.desc, self.plan,
                  self.oe, self.words, _stream())
        torch.cuda.synchronize()

    def guards_intact(self, rows):
        for k, c in self.cols.items():
            tail = c[rows:] if k != "env_ids" else c
            want = SENT_F if c.dtype == torch.float32 else (SENT_B if c.dtype == torch.uint8 else SENT_I)
            assert bool((tail == want).all()), f"column {k} written behind row {rows}"
        E = self.E
        assert bool((self.t_obs[E:] == SENT_F).all()) and bool((self.t_list[E:] == SENT_I).all())
        assert bool((self.plan[-GUARD:] == SENT_I).all())
        assert bool((self.values[E:] == SENT_F).all()) and not bool(self.stall.any())


def _scalar_values(vlogits, score, alpha):
    n = vlogits.shape[0]
    out = torch.empty(n, device=DEV)
    _lib.call("ka_scalar_value", torch.from_numpy(vlogits).to(DEV), torch.from_numpy(score).to(DEV) if alpha else None, alpha,
              out, n, _stream())
    return out.cpu().numpy()


def _run_kernel_case(E, *, T=26, alpha=0.25, obs_shape=SMALL_OBS, cap=None, every=1):
    facts = _facts_reaching_every_branch(E, T, obs_shape)
    score_norm = 76.0
    for rec in facts:                                           # the values the kernel must compute: ka_scalar_value's arithmetic
        rec["values"] = _scalar_values(rec["vlogits"], rec["score_lead"], alpha)
    # the kernel does not fill the alternating overrides (collect() does, through the buffer): the restatement without it
    want, wstats = _selfplay_host(facts, num_envs=E, obs_shape=obs_shape, action_space=SMALL_A, score_norm=score_norm, fill=False)
    total = E * T
    assert int(want["actions"].shape[0]) == total and want["size"] == T
    rig = _Rig(E, obs_shape, total if cap is None else cap, alpha, score_norm)
    rows_cap = rig.cap
    last_sync, overrides = -1, 0
    for t, rec in enumerate(facts):
        rig.step(rec)
        _same(rig.values[:E], rec["values"], "values out")
        if (t + 1) % every == 0 or t == T - 1:                    # the host's part of the deferred override, as at a sync point
            st = rig.state.cpu().numpy()
            n = int(st[_TRUNC])
            expect = [(e, p * E + e) for p in range(last_sync + 1, t + 1) for e in range(E)
                      if facts[p]["truncated"][e] and not facts[p]["terminated"][e] and p * E + e < rows_cap]
            assert n == len(expect) <= E
            tl = rig.t_list[:n].cpu().numpy()
            assert [tuple(int(v) for v in r) for r in tl] == expect          # slots in (ply, env) order
            for j, (e, row) in enumerate(expect):
                p = row // E
                _same(rig.t_obs[j], facts[p]["term_obs"][e].reshape(-1), "truncation slot")
                rig.cols["next_value_override"][row] = float(-facts[p]["term_values"][e])
            overrides += n
            rig.state[_TRUNC:_TRUNC + 1].zero_()
            last_sync = t
    st = rig.state.cpu().numpy()
    rows = min(total, rig.cap)
    assert int(st[2]) == T and int(st[_ROWS]) == rows and int(st[_DROPPED]) == total - rows and int(st[_TRUNC_DROPPED]) == 0
    assert int(st[0:2].view(np.uint64)[0]) == (1234 + T * 0x9E3779B97F4A7C15) % 2 ** 64      # the Weyl step, once per ply
    rig.guards_intact(rows)
    got = {k: v for k, v in rig.cols.items() if k != "env_ids"}
    got["observations"] = got["observations"].view(-1, *obs_shape)
    masks = torch.empty(rows + GUARD, SMALL_A, dtype=torch.bool, device=DEV)
    _lib.call("ka_unpack_mask_bits", got["legal_masks"], None, masks, rows + GUARD, SMALL_A, _stream())
    got["legal_masks"] = masks
    got["dones"], got["terminated"] = got["dones"].bool(), got["terminated"].bool()
    _same_columns({k: v[:rows] for k, v in got.items()}, want, rows)
    for k, w in TALLY_WORDS.items():                             # the tallies count every env, whether its row fitted or not
        assert int(st[w]) == wstats[k], k
    if cap is None:
        assert overrides == wstats["truncation_overrides"] > 0
    assert not st[[6, 7, 8, 9, 21, 22, 23, 25]].any()            # no sampler, refusal, guard or zero-legal flag
    assert 0 < float(st[24:25].view(np.float32)[0]) <= 60 / 76.0 + 1e-6       # word 24: bits of max |score target|
    return wstats, want


@pytest.mark.parametrize("E", [3, 64, 300, 512])
def test_selfplay_step_equals_the_host_restatement(E):
    wstats, want = _run_kernel_case(E, every=1 if E < 300 else 4)
    assert wstats["truncated"] and wstats["draws"] and wstats["wins"] and wstats["losses"]
    assert wstats["black_wins"] and wstats["white_wins"]
    assert bool((want["dones"] & want["terminated"]).any()) and bool((~want["dones"]).any())


def test_selfplay_step_odd_row_length():
    _run_kernel_case(70, obs_shape=(1, 3, 3))


def test_selfplay_step_no_blend_without_a_score_pointer():
    _run_kernel_case(64, alpha=0.0)


def test_selfplay_step_writes_nothing_past_the_reserved_rows():
    """room for five plies plus ten rows of the sixth: the drop count is the rows left out, the guard bands stay intact"""
    wstats, _ = _run_kernel_case(64, cap=5 * 64 + 10)
    assert wstats["rows"] == 26 * 64


def test_selfplay_step_raises_the_input_guards_and_the_zero_legal_latch():
    """a NaN reward on a terminated env is a label outside {-1, 0, 1, 2}; a material beyond 3.5 score_norm shows in the peak
    word; envs without a legal action, one in the first tile of 256 and two in the second, are latched by index"""
    E = 300
    facts = _facts(E, 1, 5, SMALL_OBS)
    rec = facts[0]
    rec["terminated"][3], rec["rewards"][3] = True, np.nan
    rec["material"][5] = 400
    rig = _Rig(E, SMALL_OBS, E, 0.25, 76.0)
    rig.step(rec)
    st = rig.state.cpu().numpy()
    assert st[21] == 0 and st[22] == 1 and st[23] == 0 and float(st[24:25].view(np.float32)[0]) == np.float32(400) / np.float32(76.0)
    assert st[25] == 0 and not bool(rig.stall.any())
    assert int(rig.cols["value_categories"][3]) == 3
    nl = np.ones(E, np.int32)
    nl[[7, 256, 299]] = 0
    rig2 = _Rig(E, SMALL_OBS, 3 * E, 0.25, 76.0)
    rig2.step(_facts(E, 1, 6, SMALL_OBS)[0])                      # a ply with legal actions everywhere raises nothing
    assert int(rig2.state[25]) == 0 and not bool(rig2.stall.any())
    rig2.step(_facts(E, 1, 7, SMALL_OBS)[0], nlegal=nl)
    assert int(rig2.state[25]) == 1
    assert torch.nonzero(rig2.stall).reshape(-1).tolist() == [7, 256, 299] and not bool(rig2.stall[E:].any())
    rig2.step(_facts(E, 1, 8, SMALL_OBS)[0])                      # latches: a clean ply afterwards clears neither
    assert int(rig2.state[25]) == 1 and torch.nonzero(rig2.stall).reshape(-1).tolist() == [7, 256, 299]


# ------------------------------------------------------------------ whole epochs
def _roll(N, *, alpha=0.25, max_ply=MAX_PLY, model=None, **kw):
    adapter = MultiHeadValueAdapter(score_blend_alpha=alpha) if alpha is not None else None
    kw.setdefault("seed", 4242)
    return SelfPlayRollout(model if model is not None else _model(), num_envs=N, max_ply=max_ply, value_adapter=adapter, **kw)


def _buffer(N):
    return KataGoRolloutBuffer(N, OBS, ACTION_SPACE, device=DEV)


def _values_of(roll, obs):
    """the learner's blended value of observations, by a grouped forward of its own (model 0 on every row)"""
    n = obs.shape[0]
    o = roll.group.forward(obs.to(DEV), torch.zeros(n, dtype=torch.int32, device=DEV))
    v = torch.empty(n, device=DEV)
    _lib.call("ka_scalar_value", o.value_logits.contiguous(), o.score_lead.reshape(-1).contiguous() if roll.alpha else None,
              roll.alpha, v, n, _stream())
    return v


def _term_values(roll, rec):
    out = np.full(roll.num_envs, np.nan, np.float32)
    envs = rec["terminal_envs"]
    if len(envs):
        out[envs] = _values_of(roll, rec["terminal_obs"]).cpu().numpy()
    return out


def _host_of(roll, records, final_values=None, prior=None):
    recs = [dict(r, term_values=_term_values(roll, r)) for r in records]
    return _selfplay_host(recs, num_envs=roll.num_envs, obs_shape=OBS, action_space=ACTION_SPACE, score_norm=roll.score_norm,
                          final_values=final_values, prior=prior)


def _stats_dict(stats):
    return {k: getattr(stats, k) for k in ("plies", "rows", "wins", "losses", "draws", "black_wins", "white_wins", "terminated",
                                           "truncated", "truncation_overrides")}


@pytest.mark.parametrize("N", [64, 512])
def test_recorded_epoch_equals_its_host_restatement(N):
    steps = 48
    roll = _roll(N, max_ply=16, graph=False, record=True, sync_every=8)
    buf = _buffer(N)
    stats = roll.collect(buf, steps)
    records = roll.record
    assert len(records) == steps
    nv = roll.bootstrap_values()
    final = _values_of(roll, roll.env.current().observations)
    want, wstats = _host_of(roll, records, final_values=final.cpu().numpy())
    got = buf.flatten()
    _same_columns(got, want)
    _same(nv, want["next_values"], "bootstrap values")
    assert buf.size == want["size"] == steps and buf._write_offset == steps * N
    assert _stats_dict(stats) == {k: wstats[k] for k in _stats_dict(stats)}
    assert stats.truncated > 0 and stats.truncation_overrides == stats.truncated
    assert stats.host_syncs == math.ceil(steps / 8)
    # the overrides of the truncated rows: - the blended value of a direct grouped learner forward over the recorded
    # terminal observations
    ov = got["next_value_override"].view(steps, N)
    seen = 0
    for p, rec in enumerate(records):
        envs = rec["terminal_envs"]
        if len(envs):
            _same(ov[p, torch.from_numpy(envs).to(DEV)], -_values_of(roll, rec["terminal_obs"]), "override")
            seen += len(envs)
    assert seen == stats.truncated
    # rows of the dense layout: ply p, env e at row p * N + e
    _same(got["actions"].view(steps, N)[17], records[17]["actions"], "row rule")
    _same(roll.last_values, records[-1]["values"], "last_values")


# ------------------------------------------------------------------ invariance
def _epoch(N, steps, **kw):
    roll = _roll(N, **kw)
    buf = _buffer(N)
    parts = steps if isinstance(steps, (list, tuple)) else [steps]
    stats = [roll.collect(buf, n) for n in parts]
    cols = {k: v.clone() for k, v in buf.flatten().items()}
    return roll, cols, stats, buf.size


def test_one_seed_gives_one_epoch_whatever_the_schedule():
    N, steps = 64, 64
    ref_roll, ref, ref_stats, ref_size = _epoch(N, steps, graph=False, record=True, sync_every=2)
    records = ref_roll.record
    trunc = np.stack([r["truncated"] & ~r["terminated"] for r in records])
    assert trunc.any(), "no truncation in the epoch"
    assert ref_stats[0].truncation_overrides > 0 and ref_size == steps
    for kw in (dict(graph=True, sync_every=2), dict(graph=False, sync_every=8), dict(graph=True, sync_every=8),
               dict(graph=True, sync_every=32), dict(graph=False, sync_every=32)):
        _, cols, stats, size = _epoch(N, steps, **kw)
        _same_columns(cols, ref)
        assert size == ref_size and _stats_dict(stats[0]) == _stats_dict(ref_stats[0]), kw
        assert stats[0].host_syncs == math.ceil(steps / kw["sync_every"])


@pytest.mark.parametrize("parts", [(32, 32), (31, 33)], ids=["32+32", "31+33"])
def test_one_collect_of_64_against_two(parts):
    """The fill at the end of a collect touches NaN cells of non-terminal rows only and the env goes on where it stood, so
    the split into calls leaves no trace in the buffer."""
    N = 64
    _, one, s1, size1 = _epoch(N, 64, graph=True, sync_every=8)
    _, two, s2, size2 = _epoch(N, list(parts), graph=True, sync_every=8)
    _same_columns(two, one)
    assert size1 == size2 == 64
    for k in ("wins", "losses", "draws", "black_wins", "white_wins", "terminated", "truncated", "truncation_overrides", "rows"):
        assert getattr(s1[0], k) == getattr(s2[0], k) + getattr(s2[1], k), k
    assert s1[0].truncated > 0
    ov, tm = one["next_value_override"].view(64, N), one["terminated"].view(64, N)
    assert bool(torch.isfinite(ov[parts[0] - 1][~tm[parts[0] - 1]]).all())          # the seam was filled by the second call


# ------------------------------------------------------------------ log-probs and values
def test_rows_carry_the_samplers_log_probs_and_values():
    N, alpha = 64, 0.25
    roll = _roll(N, alpha=alpha, graph=False, record=True, sync_every=4)
    buf = _buffer(N)
    roll.collect(buf, 12)
    cols = buf.flatten()
    mo = torch.zeros(N, dtype=torch.int32, device=DEV)
    for p, rec in list(enumerate(roll.record))[::3]:
        obs, bits = rec["obs"].to(DEV), rec["mask_bits"].to(DEV)
        out = roll.group.forward(obs, mo)
        a2, l2, v2 = (torch.empty(N, dtype=torch.int64, device=DEV), torch.empty(N, device=DEV), torch.empty(N, device=DEV))
        nl, fl = torch.empty(N, dtype=torch.int32, device=DEV), torch.zeros(2, dtype=torch.int32, device=DEV)
        _lib.call("ka_policy_sample", out.policy_logits.reshape(N, -1), 0, bits, MASK_WORDS, rec["seed"], out.value_logits,
                  out.score_lead.reshape(N).contiguous(), alpha, a2, l2, v2, nl, fl, N, ACTION_SPACE, _stream())
        _same(a2, rec["actions"], "actions"); _same(l2, rec["log_probs"], "log_probs"); _same(v2, rec["values"], "values")
        rows = slice(p * N, (p + 1) * N)
        _same(cols["actions"][rows], a2, "stored actions"); _same(cols["log_probs"][rows], l2, "stored log_probs")
        _same(cols["values"][rows], v2, "stored values")
        _same(cols["observations"][rows], rec["obs"], "stored observations")
    seeds = [r["seed"] for r in roll.record]
    assert all((b - a) % 2 ** 64 == 0x9E3779B97F4A7C15 for a, b in zip(seeds, seeds[1:]))


# ------------------------------------------------------------------ refresh
def test_refresh_brings_in_place_weight_edits_into_the_ply():
    m = _fresh_model(900)
    roll = SelfPlayRollout(m, num_envs=16, max_ply=MAX_PLY, graph=False, sync_every=2, seed=1)

    def logits():
        roll.reset()
        roll._ply()
        return roll._ws["logits"].clone()

    before = logits()
    with torch.no_grad():
        m.policy_conv2.bias.add_(0.5)
    stale = logits()
    assert torch.equal(before, stale)                              # the group still holds the old snapshot
    roll.refresh()
    fresh = logits()
    assert float((fresh - before).abs().max()) > 0.25


# ------------------------------------------------------------------ update
def test_ppo_update_runs_on_the_collected_buffer():
    N, steps = 64, 44
    m = _fresh_model(501)
    roll = _roll(N, model=m, graph=False, record=True, sync_every=8)
    buf = _buffer(N)
    stats = roll.collect(buf, steps)
    records = roll.record
    nv = roll.bootstrap_values()
    ppo = KataGoPPOAlgorithm(KataGoPPOParams(batch_size=256, epochs_per_batch=1), m)
    adv = ppo._advantages(buf.flatten_packed(), buf, nv, torch.device(DEV))
    # the same rows through add(): one call per ply, as the reference's loop makes them
    added = _buffer(N)
    d = lambda x, dt=None: torch.as_tensor(np.asarray(x), dtype=dt).to(DEV)  # noqa: E731
    for rec in records:
        tm, tr = d(rec["terminated"]).bool(), d(rec["truncated"]).bool()
        rw = d(rec["rewards"], torch.float32)
        cats = torch.where(tm, (1 - torch.sign(rw)).long(), torch.full_like(rw, -1).long())
        override = None
        if len(rec["terminal_envs"]):
            override = torch.full((N,), float("nan"), device=DEV)
            override[d(rec["terminal_envs"])] = -_values_of(roll, rec["terminal_obs"])
        added.add(rec["obs"].to(DEV), d(rec["actions"]), d(rec["log_probs"]), d(rec["values"]), rw, tm | tr, tm,
                  rec["mask_bits"].to(DEV), cats, d(rec["material"]).float() / roll.score_norm, next_value_override=override)
    added.fill_alternating_perspective_overrides()
    assert added.size == buf.size == steps and not added._has_env_ids
    _same_columns(buf.flatten(), added.flatten())
    adv_added = ppo._advantages(added.flatten_packed(), added, nv, torch.device(DEV))
    assert adv.shape == adv_added.shape and stats.rows == adv.numel() == steps * N
    assert torch.equal(adv, adv_added)
    metrics = ppo.update(buf, nv, value_adapter=roll.value_adapter)
    assert ppo.last_update_path == "fused"
    assert metrics and all(math.isfinite(float(x)) for x in metrics.values()), metrics
    assert buf.size == 0
    roll.refresh()
    stats2 = roll.collect(buf, 8)                                  # the next epoch goes on from the games in progress
    assert stats2.rows == 8 * N and buf.size == 8


# ------------------------------------------------------------------ errors
def test_zero_legal_row_is_raised_at_the_sync_with_the_env_named():
    roll = SelfPlayRollout(_model(), num_envs=4, max_ply=MAX_PLY, graph=False, sync_every=2, seed=3)
    b, h = S.empty_board()                                        # game.rs:1061-1124: Black to move has no legal move
    b[S.sq(0, 0)] = S.KING; b[S.sq(2, 1)] = S.KING | S.WHITE
    b[S.sq(0, 1)] = b[S.sq(1, 0)] = b[S.sq(1, 1)] = S.PAWN | S.WHITE; b[S.sq(0, 5)] = S.ROOK | S.WHITE
    roll.env.set_state(2, b, h, 0)
    buf = _buffer(4)
    with pytest.raises(RuntimeError, match=r"Environments \[2\] have zero legal actions"):
        roll.collect(buf, 2)
    assert buf.size == 0 and buf._write_offset == 0                # a chunk in which a guard fired is not committed


def test_nan_weights_are_raised_at_the_sync():
    m = _fresh_model(700)
    with torch.no_grad():
        m.policy_conv2.bias.fill_(float("nan"))
    roll = SelfPlayRollout(m, num_envs=8, max_ply=MAX_PLY, graph=False, sync_every=2, seed=3)
    buf = _buffer(8)
    with pytest.raises(RuntimeError, match="NaN in raw policy logits"):
        roll.collect(buf, 4)
    assert buf.size == 0


def test_a_buffer_with_env_ids_rows_is_refused():
    roll = SelfPlayRollout(_model(), num_envs=8, max_ply=MAX_PLY, graph=False, sync_every=2, seed=3)
    buf = _buffer(8)
    buf.reserve(8, DEV)
    buf.commit(8, 1)
    with pytest.raises(ValueError, match=r"env_ids layout.*dense \(T, N\) layout"):
        roll.collect(buf, 2)
    with pytest.raises(ValueError, match=r"dense \(T, N\) layout and the env_ids layout"):
        buf.reserve(8, env_ids=False)
    buf.clear()                                                   # an empty buffer takes the layout of its next writer
    stats = roll.collect(buf, 2)
    assert stats.rows == 16 and "env_ids" not in buf.flatten() and not buf._has_env_ids


def test_reserve_without_env_ids_against_the_default():
    dense, league = _buffer(8), _buffer(8)
    cols = dense.reserve(16, DEV, env_ids=False)
    assert not dense._has_env_ids and dense._has_next_value_override
    assert "env_ids" not in cols and "env_ids" not in dense._storage and set(cols) == {*_FIELDS, "next_value_override"}
    assert dense._write_offset == 0 and dense.size == 0 and dense._alloc_samples >= 16
    cols2 = league.reserve(16, DEV)
    assert league._has_env_ids and league._has_next_value_override and "env_ids" in cols2
    assert set(cols2) == {*_FIELDS, "env_ids", "next_value_override"}
    assert {k: (v.dtype, v.shape) for k, v in cols.items()} == {k: (v.dtype, v.shape) for k, v in cols2.items() if k != "env_ids"}
    dense.commit(16, 2)
    assert dense.size == 2 and dense._write_offset == 16
    for k in ("values", "terminated"):
        cols[k][:16] = 0
    cols["values"][8:16] = 0.5
    dense.fill_alternating_perspective_overrides()                # acts on the dense layout: -V[t + 1] into ply 0's rows
    out = dense.flatten()
    assert "env_ids" not in out
    assert bool((out["next_value_override"][:8] == -0.5).all()) and bool(torch.isnan(out["next_value_override"][8:]).all())


def test_argument_errors_on_the_device():
    m = _model()
    with pytest.raises(ValueError, match="must not exceed max_ply"):
        SelfPlayRollout(m, num_envs=8, max_ply=16, sync_every=32)
    with pytest.raises(ValueError, match="even sync_every"):
        SelfPlayRollout(m, num_envs=8, max_ply=MAX_PLY, sync_every=5, graph=True)
    with pytest.raises(ValueError, match=r"num_envs must lie in \[1, 4096\]"):
        SelfPlayRollout(m, num_envs=5000, max_ply=MAX_PLY, sync_every=4)
    roll = SelfPlayRollout(m, num_envs=8, max_ply=MAX_PLY, sync_every=4, graph=False)
    with pytest.raises(ValueError, match="steps must be positive"):
        roll.collect(_buffer(8), 0)
    with pytest.raises(ValueError, match="buffer holds"):
        roll.collect(KataGoRolloutBuffer(8, (46, 9, 9), ACTION_SPACE, device=DEV), 4)
    with pytest.raises(ValueError, match="laid out for 16 envs"):
        roll.collect(_buffer(16), 4)
    with pytest.raises(ValueError, match="device-resident"):
        roll.collect(KataGoRolloutBuffer(8, OBS, ACTION_SPACE, device="cpu"), 4)
    rig = _Rig(8, SMALL_OBS, 8, 0.0, 76.0)
    for envs, oe, norm, match in ((0, rig.oe, 76.0, "envs 0"), (5000, rig.oe, 76.0, "envs 5000"), (8, 0, 76.0, "obs_elems 0"),
                                  (8, rig.oe, 0.0, "score_norm")):
        z = torch.zeros(8 * 18, device=DEV)
        with pytest.raises(_lib.KeiseiHipError, match=match):
            _lib.call("ka_selfplay_step", rig.state, envs, z, z, z, z, z, None, 0.0, z, z, z, z, z, z, norm, z, None, rig.stall,
                      rig.values, rig.t_obs, rig.t_list, rig.desc, rig.plan, oe, rig.words, _stream())


def test_host_syncs_are_exact_and_graphs_survive_a_growing_buffer():
    N = 64
    roll = _roll(N, graph=True, sync_every=8)
    buf = _buffer(N)
    buf._ensure_capacity = _tight(buf)                             # grow at every chunk: the descriptor must follow
    for steps in (44, 8, 13, 16):
        before = buf._write_offset
        stats = roll.collect(buf, steps)
        assert stats.host_syncs == math.ceil(steps / 8)
        assert buf._write_offset - before == stats.rows == steps * N and stats.plies == steps
    assert set(roll._graphs) <= {0, 1} and roll._graphs
    cols = buf.flatten()
    assert bool((cols["actions"] >= 0).all()) and bool((cols["actions"] < ACTION_SPACE).all())
    same_roll = _roll(N, graph=False, sync_every=8)
    buf2 = _buffer(N)
    for steps in (44, 8, 13, 16):
        same_roll.collect(buf2, steps)
    _same_columns(cols, buf2.flatten())
    assert buf.size == buf2.size == 81
    del buf._ensure_capacity                                        # (the closure and the buffer name each other)


def _tight(buf):
    """an _ensure_capacity that allocates exactly what is asked, so that every reserve() moves the columns"""
    def ensure(n):
        need = buf._write_offset + n
        if need <= buf._alloc_samples:
            return
        keys = list(_FIELDS) + ["next_value_override"]
        grown = {k: buf._fresh(k, need) for k in keys}
        for k, t in grown.items():
            if k in buf._storage and buf._write_offset:
                t[:buf._write_offset] = buf._storage[k][:buf._write_offset]
        buf._storage, buf._alloc_samples = grown, need
    return ensure
