"""DynamicTrainer on the CPU: the reference's update() result (golden g11, tools/make_dynamic_golden.py), the host policy
restated from the reference's tests/test_dynamic_trainer.py on a stub store (the reference line beside each expectation),
both MatchRollout layouts, the new entry points and the collection arguments of MatchArena."""
import copy
import ctypes
import time
from collections import deque
from types import SimpleNamespace

import numpy as np
import pytest
import torch
from torch import nn

from keisei_amd import _lib
from keisei_amd.training import DynamicTrainer, MatchArena, MatchRollout
from keisei_amd.training import dynamic_trainer as dt_mod
from keisei_amd.training.dynamic_trainer import pack_mask_bits, unpack_mask_bits
from keisei_amd.training.match_arena import _referee_host, _rollout_rows_host, _side_bits
from keisei_amd.training.model_group import SEResNetGroup
from keisei_amd.training.model_registry import build_model
from keisei_amd.training.models.se_resnet import SEResNetModel, SEResNetParams

A = 11259
MP = dict(num_blocks=2, channels=32, se_reduction=8, global_pool_channels=16, policy_channels=8, value_fc_size=32,
          score_fc_size=16, obs_channels=50)


@pytest.fixture
def config():
    """the fields of the reference's DynamicConfig the trainer reads, at their defaults (keisei/config.py:103-120)"""
    return SimpleNamespace(update_epochs_per_batch=2, lr_scale=0.25, grad_clip=1.0, update_every_matches=4,
                           max_updates_per_minute=20, checkpoint_flush_every=8, disable_on_error=True, max_buffer_depth=8,
                           max_consecutive_errors=3, global_error_threshold=5, global_error_window_seconds=300.0,
                           gpu_memory_backpressure=0.9)


class Tiny(nn.Module):
    """the reference's TinyModel (tests/_helpers.py:20-35): policy and value heads on one hidden layer"""

    def __init__(self):
        super().__init__()
        self.fc = nn.Linear(50 * 81, 16)
        self.policy_head = nn.Linear(16, A)
        self.value_head = nn.Linear(16, 3)
        self.seen = []

    def forward(self, x):
        self.seen.append(self.training)
        h = torch.relu(self.fc(x.reshape(x.shape[0], -1)))
        return SimpleNamespace(policy_logits=self.policy_head(h).reshape(x.shape[0], 1, -1), value_logits=self.value_head(h))


class Store:
    def __init__(self, model):
        self.model, self.saved, self.opt, self.count, self.loaded = model, None, None, 0, None

    def load_opponent(self, entry, device):
        self.loaded = copy.deepcopy(self.model).to(device).eval()
        return self.loaded

    def load_optimizer(self, entry_id):
        return self.opt

    def save_weights(self, entry_id, sd):
        self.saved = {k: v.detach().clone() for k, v in sd.items()}
        self.model.load_state_dict(self.saved)

    def save_optimizer(self, entry_id, sd):
        self.opt = copy.deepcopy(sd)

    def increment_update_count(self, entry_id):
        self.count += 1

    def get_entry(self, entry_id):
        return SimpleNamespace(update_count=self.count, last_train_at="now" if self.count else None) if entry_id == 1 else None


ENTRY = SimpleNamespace(id=1)


def rollout(steps=6, envs=1, side=0, seed=0):
    """tests/_helpers.py:38-67"""
    g = torch.Generator().manual_seed(seed)
    actions = torch.randint(0, A, (steps, envs), generator=g)
    masks = torch.zeros(steps, envs, A, dtype=torch.bool)
    masks[:, :, 0] = True
    masks.scatter_(2, actions.unsqueeze(-1), True)
    rewards, dones = torch.zeros(steps, envs), torch.zeros(steps, envs)
    dones[-1], rewards[-1] = 1.0, 1.0
    return MatchRollout(torch.randn(steps, envs, 50, 9, 9, generator=g), actions, rewards, dones, masks,
                        torch.full((steps, envs), side, dtype=torch.long))


def trainer(config, **over):
    for k, v in over.items():
        setattr(config, k, v)
    store = Store(Tiny())
    return DynamicTrainer(store, config, 1e-3), store


# ------------------------------------------------------------------ 1. the reference's update()
def golden_rollouts(g, dtype=torch.float32):
    out = []
    for i in range(4):
        bits = g[f"r{i}.legal_mask_bits"]
        steps, envs = bits.shape[:2]
        masks = unpack_mask_bits(bits.reshape(-1, bits.shape[-1]), A).reshape(steps, envs, A)
        out.append((MatchRollout(g[f"r{i}.observations"].to(dtype), g[f"r{i}.actions"], g[f"r{i}.rewards"].to(dtype),
                                 g[f"r{i}.dones"].to(dtype), masks, g[f"r{i}.perspective"], bits), int(g[f"r{i}.side"])))
    return out


def check_weights(g, got, epochs=2, lr=2.5e-4):
    """per tensor against the fp64 result: no element further than max(2.5 d_ref, 0.05 x epochs x lr), at most 0.2 % of the
    elements further than 3e-5; integer buffers equal"""
    worst = {}
    for k, ref in g.sub("sd1.").items():
        if not ref.dtype.is_floating_point:
            assert int(got[k]) == int(ref), k
            continue
        diff = (got[k].detach().cpu().double() - ref).abs()
        bound = max(2.5 * float(g.np("dref." + k)), 0.05 * epochs * lr)
        worst[k] = (float(diff.max()), bound, float((diff > 3e-5).float().mean()))
    k = max(worst, key=lambda n: worst[n][0] / worst[n][1])
    print(f"worst tensor {k}: max diff {worst[k][0]:.3e} against {worst[k][1]:.3e}")
    for k, (mx, bound, frac) in worst.items():
        assert mx <= bound, (k, mx, bound)
        assert frac <= 2e-3, (k, frac)


def test_cpu_update_matches_the_reference(golden, config):
    g = golden("g11_dynamic")
    model = build_model("se_resnet", MP)
    model.load_state_dict(g.sub("sd0."))
    store = Store(model)
    tr = DynamicTrainer(store, config, float(g.np("learner_lr")))
    for r, side in golden_rollouts(g):
        tr.record_match(1, MatchRollout(r.observations, r.actions, r.rewards, r.dones, r.legal_masks, r.perspective), side)
    torch.manual_seed(11)
    assert tr.update(ENTRY, "cpu") is True and tr.last_update_path == "cpu"
    assert torch.allclose(tr.last_old_log_probs.double(), g["old_log_probs"], rtol=1e-4, atol=1e-4)
    check_weights(g, store.saved)
    opt = tr._optimizers[1]
    m = opt.state[opt.param_groups[0]["params"][0]]["exp_avg"]
    ref_m = g["opt.exp_avg.0"]
    assert float((m.double() - ref_m).abs().max()) <= 0.02 * float(ref_m.abs().max())
    assert abs(opt.param_groups[0]["lr"] - 2.5e-4) < 1e-12                       # test_dynamic_trainer.py:266-269


# ------------------------------------------------------------------ 2. host policy
def test_update_threshold(config):                                              # test_dynamic_trainer.py:166-176
    tr, _ = trainer(config)
    for i in range(config.update_every_matches - 1):
        tr.record_match(1, rollout(), 0)
        assert not tr.should_update(1)
    tr.record_match(1, rollout(), 0)
    assert tr.should_update(1)


def test_rate_limit_boundary_and_expiry(config, monkeypatch):                   # :182-211
    tr, _ = trainer(config)
    tr._update_timestamps = [time.monotonic()] * config.max_updates_per_minute
    assert tr.is_rate_limited()
    tr._update_timestamps = [time.monotonic() - 61.0] * config.max_updates_per_minute
    assert not tr.is_rate_limited()
    tr._update_timestamps = [940.0] * config.max_updates_per_minute
    monkeypatch.setattr(dt_mod.time, "monotonic", lambda: 1000.0)               # exactly 60 s old: kept (t >= cutoff)
    assert tr.is_rate_limited()


def test_buffer_cap_and_clear_after_update(config):                             # :400-408, :414-429
    tr, store = trainer(config, max_buffer_depth=3)
    for _ in range(5):
        tr.record_match(1, rollout(), 0)
    assert len(tr._rollout_buffers[1]) == 3
    assert tr.update(ENTRY, "cpu") is True
    assert len(tr._rollout_buffers[1]) == 0 and tr._match_counts[1] == 0
    assert any(not torch.equal(v, store.loaded.state_dict()[k]) or True for k, v in store.saved.items())
    assert store.count == 1 and tr.get_update_stats(1) == (1, "now") and tr.get_update_stats(99) == (0, None)   # :368-394


def test_update_changes_weights_and_uses_eval_then_train(config):               # :217-245, :661-693
    tr, store = trainer(config, update_every_matches=1, update_epochs_per_batch=1)
    before = copy.deepcopy(store.model.state_dict())
    tr.record_match(1, rollout(), 0)
    assert tr.update(ENTRY, "cpu") is True
    assert any(not torch.equal(before[k], store.saved[k]) for k in before)
    seen = store.loaded.seen
    assert len(seen) >= 2 and seen[0] is False and all(seen[1:])


def test_reward_signed_advantages(config, monkeypatch):                         # :435-474
    tr, _ = trainer(config, update_every_matches=1, update_epochs_per_batch=1)
    r = rollout(steps=5)
    r.rewards[-1] = -1.0
    tr.record_match(1, r, 0)
    advs = []
    real = dt_mod.ppo_clip_loss
    monkeypatch.setattr(dt_mod, "ppo_clip_loss", lambda n, o, a, **k: (advs.append(a.detach().clone()), real(n, o, a, **k))[1])
    assert tr.update(ENTRY, "cpu") is True
    assert len(advs) == 1 and bool((advs[0] < 0).any()) and bool((advs[0] == 0).any())


def test_errors_retry_disable_and_clear(config):                                # :485-507, :573-607
    tr, store = trainer(config, update_every_matches=1)
    store.load_opponent = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("simulated failure"))
    for i in range(3):
        tr.record_match(1, rollout(), 0)
        assert tr.update(ENTRY, "cpu") is False
        assert len(tr._rollout_buffers[1]) == 0 and tr._match_counts[1] == 0     # dynamic_trainer.py:266-268
        assert (1 in tr._disabled_entries) == (i == 2)
    tr.record_match(1, rollout(), 0)                                            # ignored now
    assert len(tr._rollout_buffers[1]) == 0 and tr._match_counts[1] == 0
    tr._match_counts[1] = 99
    assert tr.should_update(1) is False


def test_error_count_resets_on_success_and_reraise(config):                     # :513-541, :547-562
    tr, store = trainer(config, update_every_matches=1)
    good = store.load_opponent
    store.load_opponent = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("simulated failure"))
    for _ in range(2):
        tr.record_match(1, rollout(), 0)
        tr.update(ENTRY, "cpu")
    assert tr._error_counts[1] == 2
    store.load_opponent = good
    tr.record_match(1, rollout(), 0)
    assert tr.update(ENTRY, "cpu") is True and tr._error_counts[1] == 0
    config.disable_on_error = False
    store.load_opponent = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("simulated failure"))
    tr.record_match(1, rollout(), 0)
    with pytest.raises(RuntimeError, match="simulated failure"):
        tr.update(ENTRY, "cpu")


def test_empty_batch_returns_false(config):                                     # :613-624
    tr, _ = trainer(config)
    assert tr.update(ENTRY, "cpu") is False


def test_optimizer_saved_at_flush_interval_and_its_failure_is_not_an_error(config):      # :333-362, :630-655
    tr, store = trainer(config, update_every_matches=1, checkpoint_flush_every=2)
    tr.record_match(1, rollout(), 0)
    assert tr.update(ENTRY, "cpu") is True and store.opt is None and store.count == 1
    tr.record_match(1, rollout(seed=1), 0)
    assert tr.update(ENTRY, "cpu") is True and store.opt is not None
    tr2, store2 = trainer(config, checkpoint_flush_every=1, max_consecutive_errors=1)
    store2.save_optimizer = lambda *a: (_ for _ in ()).throw(RuntimeError("DB write failed"))
    tr2.record_match(1, rollout(), 0)
    assert tr2.update(ENTRY, "cpu") is True
    assert 1 not in tr2._disabled_entries and tr2._error_counts.get(1, 0) == 0


def test_global_disable_by_threshold_window_and_updates(config):                # :699-764
    tr, store = trainer(config, update_every_matches=1, max_consecutive_errors=100, global_error_threshold=3)
    now = time.monotonic()
    tr._global_error_timestamps = [now - 10, now - 5, now]
    tr._check_global_disable()
    assert tr.is_globally_disabled and tr.should_update(1) is False
    tr, _ = trainer(config, global_error_window_seconds=60.0)
    tr._global_error_timestamps = [now - 120, now - 5, now]
    tr._check_global_disable()
    assert not tr.is_globally_disabled
    tr, store = trainer(config, global_error_threshold=2, global_error_window_seconds=300.0)
    store.load_opponent = lambda *a, **k: (_ for _ in ()).throw(RuntimeError("model load failed"))
    for _ in range(2):
        tr.record_match(1, rollout(), 0)
        tr.update(ENTRY, "cpu")
    assert tr.is_globally_disabled and tr.should_update(1) is False


# ------------------------------------------------------------------ 3. both layouts
def test_both_rollout_layouts_give_the_same_batch(config):
    tr, _ = trainer(config)
    r = rollout(steps=5, envs=3, seed=3)
    r.perspective[:] = (torch.arange(5)[:, None] + torch.arange(3)[None, :]) % 2
    tr.record_match(1, r, 1)
    keep = (r.perspective == 1).reshape(-1)
    flat = lambda t: t.reshape(15, *t.shape[2:])[keep]  # noqa: E731
    bits = pack_mask_bits(r.legal_masks.reshape(15, A))
    assert torch.equal(unpack_mask_bits(bits, A), r.legal_masks.reshape(15, A))
    packed = MatchRollout(flat(r.observations), flat(r.actions), flat(r.rewards), flat(r.dones), None,
                          flat(r.perspective).to(torch.uint8), bits[keep])
    tr.record_match(2, packed, 1)
    a, b = tr._prepare_batch(1, "cpu"), tr._prepare_batch(2, "cpu")
    for x, y in zip(a[:4], b[:4]):
        assert torch.equal(x, y)
    assert b[4].dtype == torch.int32 and torch.equal(unpack_mask_bits(b[4], A), a[4])
    tr.record_match(2, r, 1)                                                    # mixed buffers are unpacked
    assert tr._prepare_batch(2, "cpu")[4].dtype == torch.bool


def test_packed_rollouts_train_on_the_cpu_as_the_bool_ones(golden, config):
    g = golden("g11_dynamic")
    got = []
    for packed in (False, True):
        model = build_model("se_resnet", MP)
        model.load_state_dict(g.sub("sd0."))
        store = Store(model)
        tr = DynamicTrainer(store, config, 1e-3)
        for r, side in golden_rollouts(g):
            n = r.actions.numel()
            f = lambda t: t.reshape(n, *t.shape[2:])  # noqa: E731
            tr.record_match(1, MatchRollout(f(r.observations), f(r.actions), f(r.rewards), f(r.dones),
                                            None if packed else f(r.legal_masks), f(r.perspective),
                                            f(r.legal_mask_bits) if packed else None), side)
        torch.manual_seed(5)
        assert tr.update(ENTRY, "cpu") is True
        got.append(store.saved)
    for k in got[0]:
        assert torch.equal(got[0][k], got[1][k]), k


# ------------------------------------------------------------------ 4. ABI and arguments
def test_collection_entry_points_are_exported():
    lib = ctypes.CDLL(str(_lib.library_path()))
    header = (_lib.library_path().parent.parent / "include" / "keisei_amd.h").read_text()
    for name in ("ka_arena_record_pre", "ka_arena_record_post", "ka_arena_cursor_words", "ka_dynamic_targets"):
        assert hasattr(lib, name) and name in _lib.exported_symbols() and f"int {name}(" in header, name
    assert _lib.query("ka_arena_cursor_words", 8) == 32
    assert _lib.query("ka_arena_state_words", 8) == 8 + 8 * 8                   # the state layout is unchanged


def test_side_bits_validation():
    pairs = [(0, 1), (1, 2), (2, 0)]
    assert _side_bits(None, pairs) == [0, 0, 0]
    assert _side_bits(lambda a, b: 1 if a == 0 else 2 if b == 0 else 0, pairs) == [1, 0, 2]
    assert _side_bits({0: 3, 2: 1}, pairs) == [3, 0, 1]
    with pytest.raises(ValueError, match="side bits"):
        _side_bits({1: 4}, pairs)
    with pytest.raises(ValueError, match="outside"):
        _side_bits({3: 1}, pairs)
    g = SEResNetGroup([SEResNetModel(SEResNetParams(**dict(MP, num_blocks=1))).eval()])
    with pytest.raises(ValueError, match="GPU group"):
        MatchArena(g, 8, 4, 40, sync_every=2, collect=True)


def test_record_rule_on_the_host_referee():
    """the numpy restatement of the record rule over _referee_host's seating: side bits, a zero-legal ply, the swap-in"""
    def rec(pre, rewards=None, term=None, n_legal=None):
        n = len(pre)
        return {"pre_players": np.asarray(pre, np.uint8), "rewards": np.asarray(rewards or [0.0] * n, np.float32),
                "terminated": np.asarray(term or [False] * n), "truncated": np.zeros(n, bool),
                "n_legal": np.asarray(n_legal or [5] * n)}
    recs = [rec([0, 1, 0, 0]), rec([1, 0, 1, 1], [1.0, 0, 0, 0], [True, False, False, False]),
            rec([0, 1, 0, 0], n_legal=[5, 5, 0, 5]), rec([1, 0, 1, 1])]
    kw = dict(num_slots=2, envs_per_slot=2, games_per_match=1, max_ply=50, sync_every=1)
    pairings = [(0, 1), (1, 0), (0, 0)]
    rows = _rollout_rows_host(recs, pairings, [1, 2, 3], **kw)
    assert rows[0] == [(0, 0), (1, 1)]                       # side A's movers of slot 0; done after ply 1
    assert rows[1] == [(1, 2), (1, 3)]                       # side B's movers of slot 1; ply 2 is skipped (zero legal)
    assert rows[2] == [(2, 0), (2, 1), (3, 0), (3, 1)]       # pairing 2 swapped into slot 0 at the sync after ply 1
    trace = []
    _referee_host(recs, pairings, trace=trace, **kw)
    assert trace == [{0: 0, 1: 1}, {0: 0, 1: 1}, {0: 2}, {0: 2}]
