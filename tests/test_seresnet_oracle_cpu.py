"""CPU: the decision hooks and the bf16-storage emulation of oracle.keisei_oracle.seresnet_forward, which
tests/test_hip_seresnet_batch.py uses as the reference of the HIP engine at training batch sizes.

* hooks off: bit-identical to the forward as it stood before the hooks (kept below, frozen) on the fixtures' inputs;
* a run that follows its own ReLU decisions and amax winner sets returns its own outputs and gradients exactly;
* an fp64 run that follows the decisions of an fp32 run lands within 1e-5 of its gradients where the plain comparison is
  beyond 1e-4 (one ReLU input within fp32 rounding of zero among 3.6 M at 65 boards);
* the emulation with its roundings off equals the plain forward in fp64 to 1e-12, and with them on stays within the bf16
  mode's stated distance from the fp32 fixtures (BF16_BOUNDS of test_hip_model.py: the engine sits at the same distance)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import keisei_oracle as orc

BN_EPS = orc.BN_EPS


# ------------------------------------------------------------------ the forward before the hooks, frozen
def _old_global_pool(x):
    flat = x.flatten(2)
    return torch.cat((flat.mean(dim=2), flat.amax(dim=2), flat.std(dim=2, correction=0)), dim=1)


def _old_bn(x, sd, prefix, train):
    rm, rv = sd[prefix + ".running_mean"], sd[prefix + ".running_var"]
    if train:
        rm, rv = rm.clone(), rv.clone()
    return F.batch_norm(x, rm, rv, sd[prefix + ".weight"], sd[prefix + ".bias"], training=train, momentum=0.0, eps=BN_EPS)


def _old_block(sd, prefix, x, train):
    C = x.shape[1]
    h = F.conv2d(x, sd[prefix + "conv1.weight"], padding=1)
    h = torch.relu(_old_bn(h, sd, prefix + "bn1", train))
    g = _old_global_pool(x)
    g = torch.relu(F.linear(g, sd[prefix + "global_fc.0.weight"], sd[prefix + "global_fc.0.bias"]))
    g = F.linear(g, sd[prefix + "global_fc.2.weight"], sd[prefix + "global_fc.2.bias"])
    h = h + g[:, :, None, None]
    z = _old_bn(F.conv2d(h, sd[prefix + "conv2.weight"], padding=1), sd, prefix + "bn2", train)
    sq = z.flatten(2).mean(dim=2)
    e = torch.relu(F.linear(sq, sd[prefix + "se_fc1.weight"], sd[prefix + "se_fc1.bias"]))
    e = F.linear(e, sd[prefix + "se_fc2.weight"], sd[prefix + "se_fc2.bias"])
    u = z * torch.sigmoid(e[:, :C])[:, :, None, None] + e[:, C:][:, :, None, None]
    return torch.relu(u + x)


def _old_forward(sd, obs, num_blocks, train):
    x = F.conv2d(obs, sd["input_conv.weight"], padding=1)
    x = torch.relu(_old_bn(x, sd, "input_bn", train))
    for i in range(num_blocks):
        x = _old_block(sd, f"blocks.{i}.", x, train)
    p = F.conv2d(x, sd["policy_conv1.weight"])
    p = torch.relu(_old_bn(p, sd, "policy_bn1", train))
    p = F.conv2d(p, sd["policy_conv2.weight"], sd["policy_conv2.bias"])
    pool = _old_global_pool(x)
    v = torch.relu(F.linear(pool, sd["value_fc1.weight"], sd["value_fc1.bias"]))
    v = F.linear(v, sd["value_fc2.weight"], sd["value_fc2.bias"])
    s = torch.relu(F.linear(pool, sd["score_fc1.weight"], sd["score_fc1.bias"]))
    s = F.linear(s, sd["score_fc2.weight"], sd["score_fc2.bias"])
    return p.permute(0, 2, 3, 1), v, s


MID = [("s6x128.", orc.NetShape(6, 128)), ("s3x256.", orc.NetShape(3, 256))]


def _fixture_cases(golden):
    g = golden("g2_model_tiny")
    sd = g.sub("sd.")
    yield "tiny randn", sd, g["randn.obs"], 2
    yield "tiny board", sd, g["board.obs"], 2
    g = golden("g2_model_mid16")
    for tag, shape in MID:
        yield tag, orc.init_like_state_dict(shape), g[tag + "obs"], shape.num_blocks


def test_hooks_off_is_the_forward_as_it_was(golden):
    for label, sd, obs, nb in _fixture_cases(golden):
        for train in (False, True):
            with torch.no_grad():
                new = orc.seresnet_forward(sd, obs, nb, train, momentum=0.0)
                old = _old_forward(sd, obs, nb, train)
            for a, b in zip(new, old):
                assert torch.equal(a, b), (label, train)


def _run(sd, obs, nb, dt, **kw):
    """outputs and parameter gradients of (p * cp).sum() / B + (v * cv).sum() + (s * cs).sum() in dt, train mode"""
    B = obs.shape[0]
    leaves = {k: v.to(dt).requires_grad_(True) for k, v in sd.items() if v.dtype.is_floating_point and "running" not in k}
    live = {k: (v.to(dt) if v.dtype.is_floating_point else v.clone()) for k, v in sd.items()}
    live.update(leaves)
    cp, cv, cs = orc.closed_form_cotangents(B)
    p, v, s = orc.seresnet_forward(live, obs.to(dt), nb, True, momentum=0.0, **kw)
    loss = (p * cp.to(dt)).sum() / B + (v * cv.to(dt)).sum() + (s * cs.to(dt)).sum()
    grads = dict(zip(leaves, torch.autograd.grad(loss, list(leaves.values()))))
    return (p.detach(), v.detach(), s.detach()), grads


def _decisions(relu_taps, pool_taps):
    return [a > 0 for a in relu_taps], [f == f.amax(dim=2, keepdim=True) for f in pool_taps]


def _rel_l2(grads, ref):
    out = []
    for n, r in ref.items():
        rn = float(r.double().norm())
        if rn > 0:
            out.append(float((grads[n].double() - r.double()).norm()) / rn)
    return sorted(out)


def test_following_its_own_decisions_changes_nothing(golden):
    for label, sd, obs, nb in _fixture_cases(golden):
        for dt in (torch.float32, torch.float64):
            rt, pt = [], []
            out, grads = _run(sd, obs, nb, dt, relu_inputs=rt, pool_inputs=pt)
            assert len(rt) == 1 + 4 * nb + 3 and len(pt) == nb + 1, (len(rt), len(pt))
            assert pt[0].shape == (obs.shape[0], sd["input_conv.weight"].shape[0], 81)
            rm, pw = _decisions(rt, pt)
            out2, grads2 = _run(sd, obs, nb, dt, relu_masks=rm, pool_winners=pw)
            for a, b in zip(out, out2):
                assert torch.equal(a, b), (label, dt)
            for n in grads:
                assert torch.equal(grads[n], grads2[n]), (label, dt, n)


def test_fp64_following_an_fp32_run_reaches_its_gradients():
    """2x128 at 65 boards (board_like_obs seed 65): the fp32 and the fp64 run of the oracle differ in a ReLU decision, and that
    one decision is the whole distance between their gradients."""
    shape, B = orc.NetShape(2, 128), 65
    sd = orc.init_like_state_dict(shape)
    obs = orc.board_like_obs(B, seed=B)
    rt, pt = [], []
    _, g32 = _run(sd, obs, 2, torch.float32, relu_inputs=rt, pool_inputs=pt)
    rt64, pt64 = [], []
    _, g64 = _run(sd, obs, 2, torch.float64, relu_inputs=rt64, pool_inputs=pt64)
    rm, pw = _decisions(rt, pt)
    n_relu = sum(int(((a > 0) != (b > 0)).sum()) for a, b in zip(rt, rt64))
    n_pool = sum(int(((w != (f == f.amax(dim=2, keepdim=True))).any(dim=2)).sum()) for w, f in zip(pw, pt64))
    plain = _rel_l2(g32, g64)
    _, g64f = _run(sd, obs, 2, torch.float64, relu_masks=rm, pool_winners=pw)
    followed = _rel_l2(g32, g64f)
    print(f"2x128 B=65: {n_relu} ReLU decisions and {n_pool} amax winner sets differ; worst relative L2 plain {plain[-1]:.2e}, "
          f"followed {followed[-1]:.2e}")
    assert n_relu + n_pool >= 1
    assert plain[-1] > 1e-4, plain[-1]
    assert followed[-1] <= 1e-5, followed[-1]


def test_emulation_without_rounding_is_the_plain_forward(golden):
    for label, sd, obs, nb in _fixture_cases(golden):
        sd64 = {k: (v.double() if v.dtype.is_floating_point else v.clone()) for k, v in sd.items()}
        for train in (False, True):
            with torch.no_grad():
                ref = orc.seresnet_forward(sd64, obs.double(), nb, train, momentum=0.0)
                emu = orc.seresnet_forward(sd64, obs.double(), nb, train, momentum=0.0, bf16_storage=True, rounding=False)
            for a, b in zip(emu, ref):
                assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), (label, train)


def test_gemm_form_of_the_convolutions_is_conv2d():
    """On a GPU the oracle takes its convolutions as one matrix product over gathered taps: same sums as F.conv2d, values and
    gradients, in float64 to rounding."""
    g = torch.Generator().manual_seed(3)
    for (O, C, k, pad, with_bias) in ((24, 50, 3, 1, False), (16, 24, 3, 1, False), (8, 24, 1, 0, False), (139, 8, 1, 0, True)):
        x = torch.randn(5, C, 9, 9, generator=g, dtype=torch.float64, requires_grad=True)
        w = torch.randn(O, C, k, k, generator=g, dtype=torch.float64, requires_grad=True)
        b = torch.randn(O, generator=g, dtype=torch.float64, requires_grad=True) if with_bias else None
        cot = torch.randn(5, O, 9, 9, generator=g, dtype=torch.float64)
        leaves = [t for t in (x, w, b) if t is not None]
        ref = F.conv2d(x, w, b, padding=pad)
        got = orc._conv_gemm(x, w, b, pad)
        assert got.shape == ref.shape and float((got - ref).abs().max()) <= 1e-12 * float(ref.abs().max())
        for gr, gg in zip(torch.autograd.grad((ref * cot).sum(), leaves), torch.autograd.grad((got * cot).sum(), leaves)):
            assert float((gg - gr).abs().max()) <= 1e-12 * float(gr.abs().max())


# the eval / train entries of BF16_BOUNDS in test_hip_model.py (policy max |error| / |logit|max against the fp32 fixture)
EMU_BOUNDS = {"s6x128.": (0.009, 0.030), "s3x256.": (0.006, 0.020)}


@pytest.mark.parametrize("tag,shape", MID)
def test_emulation_with_rounding_is_at_the_bf16_modes_distance(golden, tag, shape):
    g = golden("g2_model_mid16")
    sd = orc.init_like_state_dict(shape)
    obs = g[tag + "obs"]
    for train, bound in zip((False, True), EMU_BOUNDS[tag]):
        with torch.no_grad():
            pol, val, sco = orc.seresnet_forward(sd, obs, shape.num_blocks, train, momentum=0.0, bf16_storage=True)
            assert torch.equal(pol, orc.seresnet_policy_bf16_storage(sd, obs, shape.num_blocks, train))
        ref = g[tag + ("train.policy" if train else "eval.policy")]
        e = float((pol - ref).abs().max()) / float(ref.abs().max())
        print(f"{tag} emulation train={train}: policy max diff / |logit|max {e:.4f} (bound {bound})")
        assert val.shape == (obs.shape[0], 3) and sco.shape == (obs.shape[0], 1)
        assert 0 < e <= bound, (tag, train, e)
