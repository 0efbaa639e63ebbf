"""DynamicTrainer on the GPU: the fused fp32 update against the reference's fp64 result (golden g11), bf16, the guard
flags of the update, and the closed loop arena round -> record_match -> update on the attached group -> next round."""
import copy
from types import SimpleNamespace

import pytest
import torch

from keisei_amd.shogi_gym import VecEnv
from keisei_amd.training import DynamicTrainer, MatchArena, MatchRollout
from keisei_amd.training.model_group import SEResNetGroup
from keisei_amd.training.model_registry import build_model
from keisei_amd.training.models.se_resnet import SEResNetModel, SEResNetParams
from oracle import keisei_oracle as orc
from test_dynamic_trainer_cpu import ENTRY, MP, Store, check_weights, golden_rollouts

pytestmark = pytest.mark.gpu
DEV = "cuda"
SHAPE = orc.NetShape(2, 128, 8, 64, 16, 128, 64)


def _config(**over):
    c = SimpleNamespace(update_epochs_per_batch=2, lr_scale=0.25, grad_clip=1.0, update_every_matches=4,
                        max_updates_per_minute=20, checkpoint_flush_every=8, disable_on_error=True, max_buffer_depth=8,
                        max_consecutive_errors=3, global_error_threshold=5, global_error_window_seconds=300.0,
                        gpu_memory_backpressure=0.9)
    c.__dict__.update(over)
    return c


def _flat_device(r: MatchRollout) -> MatchRollout:
    """the arena's layout: flat rows on the device, packed masks"""
    n = r.actions.numel()
    f = lambda t: t.reshape(n, *t.shape[2:]).to(DEV)  # noqa: E731
    return MatchRollout(f(r.observations), f(r.actions), f(r.rewards), f(r.dones), None, f(r.perspective).to(torch.uint8),
                        f(r.legal_mask_bits))


def _trainer(golden, use_amp=False, **over):
    g = golden("g11_dynamic")
    model = build_model("se_resnet", MP)
    model.load_state_dict(g.sub("sd0."))
    store = Store(model)
    tr = DynamicTrainer(store, _config(**over), float(g.np("learner_lr")), use_amp=use_amp)
    for r, side in golden_rollouts(g):
        tr.record_match(1, _flat_device(r), side)
    return g, tr, store


# ------------------------------------------------------------------ 8. update parity
def test_fused_update_matches_the_reference(golden):
    g, tr, store = _trainer(golden)
    torch.manual_seed(3)
    assert tr.update(ENTRY, DEV) is True
    assert tr.last_update_path == "fused"
    old = tr.last_old_log_probs.cpu().double()
    print("old_log_probs: max abs diff", float((old - g["old_log_probs"]).abs().max()))
    assert torch.allclose(old, g["old_log_probs"], rtol=1e-4, atol=1e-4)
    check_weights(g, store.saved)
    assert store.count == 1 and len(tr._rollout_buffers[1]) == 0
    opt = tr._optimizers[1]
    assert all(v.device.type == "cpu" for s in opt.state.values() for v in s.values() if isinstance(v, torch.Tensor))


def test_bf16_update_runs_and_moves_the_weights(golden):
    g, tr, store = _trainer(golden, use_amp=True)
    assert tr.update(ENTRY, DEV) is True and tr.last_update_path == "fused"
    sd0 = g.sub("sd0.")
    assert all(bool(torch.isfinite(v).all()) for v in store.saved.values() if v.dtype.is_floating_point)
    assert any(not torch.equal(store.saved[k].cpu(), sd0[k]) for k in sd0 if sd0[k].dtype.is_floating_point)
    assert store.loaded._amp_enabled is False               # the model's own autocast setting is put back


# ------------------------------------------------------------------ 10. error policy
def test_action_outside_the_action_space_is_an_error_not_a_fault(golden):
    g, tr, store = _trainer(golden)
    bad = tr._rollout_buffers[1][0][0]
    rows = (bad.perspective == tr._rollout_buffers[1][0][1]).nonzero(as_tuple=True)[0]
    bad.actions[rows[0]] = 11259 + 5
    assert tr.update(ENTRY, DEV) is False
    assert tr._error_counts[1] == 1 and len(tr._rollout_buffers[1]) == 0 and tr._match_counts[1] == 0
    assert store.saved is None and 1 not in tr._optimizers
    sd0 = g.sub("sd0.")                                       # the guard flags vetoed every optimiser step
    for k, v in store.loaded.state_dict().items():
        if v.dtype.is_floating_point and "running" not in k:
            assert torch.equal(v.cpu(), sd0[k]), k


# ------------------------------------------------------------------ 9. the loop closes
def test_the_loop_closes_on_the_device():
    ms = []
    for k in range(3):
        m = SEResNetModel(SEResNetParams(**SHAPE.__dict__))
        m.load_state_dict(orc.init_like_state_dict(SHAPE, salt=29 * k + 5), strict=True)
        ms.append(m.to(DEV).eval())
    group = SEResNetGroup(ms)
    arena = MatchArena(group, 16, 4, 30, sync_every=2, graph=True, seed=5, collect=True)
    pairings = [(0, 1), (1, 2), (2, 1), (1, 0)]
    bits = {0: 2, 1: 1, 2: 2, 3: 1}                           # model 1 is the Dynamic entry, on whichever side it plays
    results, stats = arena.run_round(pairings, games_per_match=4, trainable=bits)
    store = Store(None)
    store.save_weights = lambda eid, sd: setattr(store, "saved", {k: v.detach().clone() for k, v in sd.items()})
    store.load_opponent = lambda *a: (_ for _ in ()).throw(AssertionError("an attached entry is not loaded from the store"))
    tr = DynamicTrainer(store, _config(), 1e-3)
    tr.attach_group(group, {1: 1})
    for r, b in zip(results, bits.values()):
        assert r.rollout is not None
        for k in ("observations", "actions", "rewards", "dones", "perspective", "legal_mask_bits"):
            assert getattr(r.rollout, k).device.type == "cuda", k          # nothing of the rollout lives on the host
        tr.record_match(1, r.rollout, b - 1)
    assert tr.should_update(1) and stats.rollout_rows == sum(r.rollout.actions.shape[0] for r in results)

    env = VecEnv(6, 30, "katago", "spatial", output="torch")
    obs = env.reset().observations.clone()
    idx = torch.tensor([0, 1, 2, 0, 1, 2], dtype=torch.int32, device=DEV)
    before = group.forward(obs, idx).policy_logits.clone()
    w_before = {k: v.clone() for k, v in ms[1].state_dict().items()}
    assert tr.update(ENTRY, DEV) is True and tr.last_update_path == "fused"
    after = group.forward(obs, idx).policy_logits
    changed = (after != before).reshape(6, -1).any(dim=1).cpu().tolist()
    assert changed == [False, True, False, False, True, False]
    assert not ms[1].training and all(not m.training for m in ms[1].modules())
    assert any(not torch.equal(w_before[k], v) for k, v in ms[1].state_dict().items())
    for k, v in ms[1].state_dict().items():
        assert torch.equal(store.saved[k], v), k
    again, stats2 = arena.run_round(pairings, games_per_match=4, trainable=bits)      # the same captured graph
    assert stats2.pairings_completed == 4 and all(r.rollout is not None for r in again)
    assert [(r.a_wins, r.b_wins, r.draws, r.plies) for r in again] != [(r.a_wins, r.b_wins, r.draws, r.plies) for r in results] \
        or not torch.equal(again[0].rollout.actions, results[0].rollout.actions)
