"""SEResNetGroup on the CPU: validation, the per-model loop and the C ABI of the grouped kernels."""
import ctypes

import pytest
import torch

from keisei_amd import _lib
from keisei_amd.training.model_group import SEResNetGroup
from keisei_amd.training.models.se_resnet import SEResNetModel, SEResNetParams
from oracle import keisei_oracle as orc

TINY = dict(num_blocks=2, channels=32, se_reduction=8, global_pool_channels=16, policy_channels=8,
            value_fc_size=32, score_fc_size=16, obs_channels=50)
GROUPED = ("ka_tower_eval_grouped_supported", "ka_stem_eval_grouped", "ka_tower_eval_grouped", "ka_heads_eval_grouped")


def _model(salt, **over):
    p = SEResNetParams(**{**TINY, **over})
    m = SEResNetModel(p)
    m.load_state_dict(orc.init_like_state_dict(orc.NetShape(**p.__dict__), salt=salt), strict=True)
    return m.eval()


def test_grouped_entry_points_are_exported():
    lib = ctypes.CDLL(str(_lib.library_path()))
    for name in GROUPED:
        assert hasattr(lib, name), name
        assert name in _lib.exported_symbols(), name
    assert _lib.query("ka_tower_eval_grouped_supported", 128, 64, 16, _lib.DTYPE_BF16) == 1
    assert _lib.query("ka_tower_eval_grouped_supported", 256, 128, 16, _lib.DTYPE_BF16) == 1
    assert _lib.query("ka_tower_eval_grouped_supported", 64, 32, 8, _lib.DTYPE_BF16) == 0
    assert _lib.query("ka_tower_eval_grouped_supported", 128, 64, 16, _lib.DTYPE_F32) == 0


def test_mismatched_params_are_refused():
    with pytest.raises(ValueError, match="SEResNetParams"):
        SEResNetGroup([_model(0), _model(1, policy_channels=4)])
    with pytest.raises(ValueError, match="at least one"):
        SEResNetGroup([])


def test_out_of_range_model_idx_is_refused_with_check():
    grp = SEResNetGroup([_model(0), _model(1)])
    obs = torch.randn(3, 50, 9, 9)
    with pytest.raises(ValueError, match="out of range"):
        grp.forward(obs, torch.tensor([0, 2, 1]))
    with pytest.raises(ValueError, match="out of range"):
        grp.forward(obs, torch.tensor([0, -2, 1]))
    with pytest.raises(ValueError, match="shape"):
        grp.forward(obs, torch.tensor([0, 1]))


def test_cpu_loop_equals_each_models_own_forward_bit_for_bit():
    models = [_model(s) for s in range(3)]
    grp = SEResNetGroup(models)
    g = torch.Generator().manual_seed(0)
    obs = torch.randn(9, 50, 9, 9, generator=g)
    idx = torch.tensor([2, 0, -1, 2, 2, 0, -1, 0, 2])
    out = grp.forward(obs, idx)
    assert out.policy_logits.shape == (9, 9, 9, 139) and out.value_logits.shape == (9, 3) and out.score_lead.shape == (9, 1)
    with torch.no_grad():
        for k, m in enumerate(models):
            rows = (idx == k).nonzero(as_tuple=True)[0]
            if rows.numel() == 0:
                continue
            o = m(obs[rows])
            assert torch.equal(out.policy_logits[rows], o.policy_logits)
            assert torch.equal(out.value_logits[rows], o.value_logits)
            assert torch.equal(out.score_lead[rows], o.score_lead)
    # the models are different: the same board under two models gives clearly different outputs
    with torch.no_grad():
        a, b = models[0](obs[:1]), models[2](obs[:1])
    assert float((a.policy_logits - b.policy_logits).abs().max()) > 1e-2


def test_unseated_rows_are_zero():
    grp = SEResNetGroup([_model(0), _model(1)])
    obs = torch.randn(4, 50, 9, 9)
    out = grp.forward(obs, torch.tensor([-1, 1, -1, 0]))
    for t in (out.policy_logits, out.value_logits, out.score_lead):
        assert torch.count_nonzero(t[[0, 2]]) == 0
        assert torch.count_nonzero(t[[1, 3]]) > 0


def test_cpu_select_actions_legal_and_consistent():
    grp = SEResNetGroup([_model(0), _model(1)])
    g = torch.Generator().manual_seed(1)
    obs = torch.randn(5, 50, 9, 9, generator=g)
    idx = torch.tensor([0, 1, -1, 1, 0])
    masks = torch.rand(5, 81 * 139, generator=g) < 0.05
    masks[2] = False                                      # an unseated row may have no legal action
    actions, logp = grp.select_actions(obs, masks, idx, seed=7)
    assert actions[2] == -1 and logp[2] == 0
    seated = [0, 1, 3, 4]
    assert bool(masks[seated, actions[seated]].all())
    logits = grp.forward(obs, idx).policy_logits.reshape(5, -1)
    ref = torch.log_softmax(logits.masked_fill(~masks, float("-inf")), dim=-1)
    assert torch.allclose(logp[seated], ref[seated, actions[seated]], atol=1e-5)
    bits = torch.zeros(5, (81 * 139 + 31) // 32, dtype=torch.int64)
    nz = masks.nonzero()
    bits.index_put_((nz[:, 0], nz[:, 1] // 32), torch.ones(len(nz), dtype=torch.int64) << (nz[:, 1] % 32), accumulate=True)
    packed = bits.to(torch.int32)
    a2, _ = grp.select_actions(obs, packed, idx, seed=7)
    assert torch.equal(actions, a2)
    masks[1] = False
    with pytest.raises(RuntimeError, match="zero legal actions"):
        grp.select_actions(obs, masks, idx, seed=7)
