"""Pins oracle.keisei_oracle.transformer_forward, the functional restatement the batch-size GPU tests
(test_hip_transformer_batch.py) use as their reference, against the CPU TransformerModel in fp64 (outputs and autograd
gradients), against the reference-generated g9 fixtures, and pins where it applies its explicit dropout masks."""
import math

import pytest
import torch

from keisei_amd.training.model_registry import build_model
from oracle import keisei_oracle as orc

CONFIGS = [("d32h4L2.", {"d_model": 32, "nhead": 4, "num_layers": 2}), ("d64h2L1.", {"d_model": 64, "nhead": 2, "num_layers": 1}),
           ("d256h8L1.", {"d_model": 256, "nhead": 8, "num_layers": 1})]
FIXTURE = {"d32h4L2.": "g9_transformer", "d64h2L1.": "g9_transformer", "d256h8L1.": "g9_transformer_d256"}


def _model64(p):
    """The CPU TransformerModel in fp64 with the fixtures' hash weights, train mode, every dropout at 0."""
    m = build_model("transformer", p)
    m.load_state_dict(orc.hash_fill(m.state_dict()), strict=True)
    m = m.double().train()
    for mod in m.modules():
        if isinstance(mod, torch.nn.Dropout):
            mod.p = 0.0
        if isinstance(mod, torch.nn.MultiheadAttention):
            mod.dropout = 0.0
    return m


def _oracle_grads(m, p, obs, cp, cv, masks=None):
    """Oracle outputs and gradients of (policy * cp).sum() / B + (value * cv).sum() over leaves sharing m's storage."""
    leaves = {n: t.detach().requires_grad_(True) for n, t in m.named_parameters()}
    pol, val = orc.transformer_forward(leaves, obs, p["num_layers"], p["nhead"], drop_masks=masks)
    loss = (pol * cp).sum() / obs.shape[0] + (val * cv).sum()
    return pol.detach(), val.detach(), dict(zip(leaves, torch.autograd.grad(loss, list(leaves.values()))))


def _model_grads(m, obs, cp, cv):
    pol, val = m(obs)
    loss = (pol * cp).sum() / obs.shape[0] + (val * cv).sum()
    names = [n for n, _ in m.named_parameters()]
    return pol.detach(), val.detach(), dict(zip(names, torch.autograd.grad(loss, [t for _, t in m.named_parameters()])))


def _rel(a, b):
    return float((a - b).norm() / (b.norm() + 1e-300))


@pytest.mark.parametrize("tag,p", CONFIGS)
def test_oracle_matches_fp64_model_and_fixtures(golden, tag, p):
    g = golden(FIXTURE[tag])
    m = _model64(p)
    obs = g[tag + "obs"].double()
    B = obs.shape[0]
    cp = orc._hash_uniform(B * 11259, 7101).float().double().reshape(B, 11259)      # the fixtures' fp32 cotangents
    cv = orc._hash_uniform(B, 7102).float().double().reshape(B, 1)
    pol, val, grads = _oracle_grads(m, p, obs, cp, cv)
    # the CPU model in fp64: outputs and every autograd gradient
    mpol, mval, mgrads = _model_grads(m, obs, cp, cv)
    assert _rel(pol, mpol) < 1e-12 and _rel(val, mval) < 1e-12
    worst = max(_rel(grads[n], mgrads[n]) for n in mgrads)
    assert worst < 1e-12, worst
    # the fixtures: fp32 outputs of the reference at their tolerance ...
    for key, got in (("eval.policy", pol), ("eval.value", val), ("train.policy", pol), ("train.value", val)):
        assert torch.allclose(got.float(), g[tag + key], rtol=1e-4, atol=2e-5), key
    # ... their fp64 gradient norms, and the stored gradients: fp64 gradients rounded to fp32, so the oracle's are rounded
    # the same way (left: one-ulp flips of a few elements whose fp64 values differ in the last bits)
    norms = dict(zip(list(g.np(tag + "grad_names")), g.np(tag + "grad_norms64")))
    assert set(norms) == set(grads)
    for n, ref_norm in norms.items():
        assert abs(float(grads[n].norm()) - ref_norm) <= 1e-12 * ref_norm, n
    checked = 0
    for n, got in grads.items():
        for key, o in ((f"{tag}grad64.{n}", got), (f"{tag}grad64.{n}[:8]", got[:8])):
            if key in g:
                assert _rel(o.float().double(), g[key].double()) < 1e-10, key
                checked += 1
    assert checked >= 10


class _Scale(torch.nn.Module):
    """Stands in for an nn.Dropout of the CPU model: multiplies by a fixed per-element mask."""

    def __init__(self, mask):
        super().__init__()
        self.mask = mask

    def forward(self, x):
        return x * self.mask.reshape(x.shape)


@pytest.mark.parametrize("tag,p", CONFIGS[:2])
def test_oracle_dropout_masks_sit_where_the_encoder_layer_drops(tag, p):
    """Masks in the oracle against the same masks put in place of dropout1 / dropout / dropout2 of the fp64 CPU model
    (outputs and gradients); masks of ones give the no-dropout result exactly."""
    m = _model64(p)
    B, d = 3, p["d_model"]
    gen = torch.Generator().manual_seed(11)
    obs = torch.cat([orc.board_like_obs(2, seed=4), torch.randn(1, 50, 9, 9, generator=gen)]).double()
    cp, cv = torch.randn(B, 11259, generator=gen).double(), torch.randn(B, 1, generator=gen).double()

    def mask(n):
        return (torch.rand(B * 81, n, generator=gen) >= 0.1).double() / 0.9

    masks = [(mask(d), mask(4 * d), mask(d)) for _ in range(p["num_layers"])]
    pol0, val0, _ = _oracle_grads(m, p, obs, cp, cv)
    ones = [tuple(torch.ones_like(t) for t in ms) for ms in masks]
    pol1, val1, _ = _oracle_grads(m, p, obs, cp, cv, ones)
    assert torch.equal(pol0, pol1) and torch.equal(val0, val1)
    pol, val, grads = _oracle_grads(m, p, obs, cp, cv, masks)
    assert _rel(pol, pol0) > 1e-3                                   # the masks do something
    for lyr, (m1, mf, m2) in zip(m.encoder.layers, masks):
        lyr.dropout1, lyr.dropout, lyr.dropout2 = _Scale(m1), _Scale(mf), _Scale(m2)
    mpol, mval, mgrads = _model_grads(m, obs, cp, cv)
    assert _rel(pol, mpol) < 1e-12 and _rel(val, mval) < 1e-12
    worst = max(_rel(grads[n], mgrads[n]) for n in mgrads)
    assert worst < 1e-12, worst


@pytest.mark.parametrize("tag,p", CONFIGS[:2])
def test_oracle_bf16_storage_is_a_bf16_sized_perturbation(tag, p):
    """bf16_storage rounds something (the result moves) and only at bf16 scale; with it off the fp32 oracle stays within
    fp32 rounding of the fp64 one."""
    m = _model64(p)
    sd = {n: t.detach() for n, t in m.named_parameters()}
    obs = orc.board_like_obs(4, seed=8).double()
    pol, val = orc.transformer_forward(sd, obs, p["num_layers"], p["nhead"])
    pq, vq = orc.transformer_forward(sd, obs, p["num_layers"], p["nhead"], bf16_storage=True)
    e = float((pq - pol).abs().max()) / float(pol.abs().max())
    assert 2.0 ** -12 < e < 0.03, e
    p32, _ = orc.transformer_forward({n: t.float() for n, t in sd.items()}, obs.float(), p["num_layers"], p["nhead"])
    assert float((p32.double() - pol).abs().max()) / float(pol.abs().max()) < 1e-5
    assert math.isfinite(float(vq.abs().max()))
