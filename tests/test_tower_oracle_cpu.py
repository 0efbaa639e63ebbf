"""CPU side of the tower oracle (tests/tower_helpers.py): the float64 block, stem and heads references equal the model
(oracle/keisei_oracle.py, itself pinned to SEResNetModel) at shapes the end-to-end tests do not use, every exact case meets the
conditions under which a kernel must be exact to the bit, every tier-2 case goes through one rounding only, the case lists
cover every accepted edge, and every mutant -- one wrong line of a reference -- is caught by them."""
import math

import pytest
import torch

import tower_helpers as th
from tower_helpers import F32, F64
from oracle import keisei_oracle as orc

ATOL = 1e-11       # float64 against float64 through two blocks: BatchNorm folded into (scale, shift) against F.batch_norm


def same(a, b, what):
    assert a.shape == b.shape, what
    assert float((a - b).abs().max()) <= ATOL * max(1.0, float(b.abs().max())), (what, float((a - b).abs().max()))


def nchw(t):
    return t.permute(0, 2, 1).reshape(t.shape[0], t.shape[2], 9, 9)


@pytest.mark.parametrize("shape", [orc.NetShape(2, 128, 8, 24, 7, 65, 3), orc.NetShape(2, 128, 8, 64, 16, 128, 64, 46)],
                         ids=["G24-R16-P7-V65-S3", "cin46"])
def test_references_equal_the_model_in_float64(shape):
    """stem_ref -> tower_ref -> heads_ref with the roundings off against seresnet_forward, and block by block against
    block_forward, in eval mode"""
    sd = {k: (v.double() if v.is_floating_point() else v) for k, v in orc.init_like_state_dict(shape, salt=5).items()}
    B, C = 3, shape.channels
    G, R = shape.global_pool_channels, C // shape.se_reduction
    obs = torch.randn(B, shape.obs_channels, 9, 9, generator=torch.Generator().manual_seed(3), dtype=F64)
    stem, blocks, head = th.model_parts(sd, shape)
    mo = (0,) * B
    s = th.stem_ref(th.Stem("model", C, shape.obs_channels, 1, mo, (stem,), obs), F64, rnd=False)
    pool_in = torch.cat([th.pool3(s["x"], F64), torch.zeros(B, C, dtype=F64)], 1)
    same(s["pool"], pool_in, "stem pool")
    t = th.tower_ref(th.Tower("model", "model", C, G, R, shape.num_blocks, 1, mo, (blocks,), s["x"], pool_in), F64, rnd=False, trace=True)
    x = nchw(s["x"])
    for i, tr in enumerate(t["trace"]):
        x = orc.block_forward(sd, f"blocks.{i}.", x, False)
        same(nchw(tr["out"]), x, f"block {i}")
    same(t["pool"][:, :3 * C], orc.global_pool(x), "tower pool")
    h = th.heads_ref(th.Heads("model", C, shape.policy_channels, shape.value_fc_size, shape.score_fc_size, 1, mo, (head,), t["x"], t["pool"]), F64)
    pol, val, sco = orc.seresnet_forward(sd, obs, shape.num_blocks, False)
    same(h["logits"], pol, "policy"); same(h["value"], val, "value"); same(h["score"], sco, "score")
    assert float(pol.abs().max()) > 0.1 and float(val.abs().max()) > 0.01


def test_case_lists_cover_every_accepted_edge():
    for C in (128, 256):
        for kind in ("conv", "se"):
            cs = [k for k in th.EXACT_TOWER if k[0] == kind and k[1] == C]
            assert {k[2] for k in cs} == set(th.GS) and {k[3] for k in cs} == set(th.RS)
            assert {k[4] for k in cs} == {1, 5} and {k[5] for k in cs} == {1, 3} and {k[6] for k in cs} == {1, 3}
        assert {k[2] for k in th.TIER2_GP if k[1] == C} == set(th.GS) and {k[3] for k in th.TIER2_SE if k[1] == C} == set(th.RS)
        assert {k[1] for k in th.STEM_CASES if k[0] == C} == set(th.CINS)
        hs = [k for k in th.HEADS_CASES if k[0] == C]
        assert {k[1] for k in hs} == {1, 7, 32} and {k[2:] for k in hs} == {(1, 1), (3, 65), (200, 130), (512, 512)}
    for kind in ("conv", "se"):                    # ka_tower_eval runs the K = 1 cases at C = 256 beside the grouped form
        assert [k for k in th.EXACT_TOWER if k[0] == kind and k[1] == 256 and k[5] == 1]
    for key in th.EXACT_TOWER:
        c = th.exact_tower_case(*key)
        assert c.B <= 7 and c.nb <= 3
        if c.K == 3 and c.B == 5:
            assert len(set(c.model_of)) == 3 and list(c.model_of) != sorted(c.model_of)
    h = th.heads_case(*th.HEADS_CASES[0])
    assert h.B <= 7 and -1 in h.model_of and h.K in h.model_of and {m for m in h.model_of if th.seated(m, h.K)} == {0, 1, 2}


@pytest.mark.parametrize("key", th.EXACT_TOWER, ids=lambda k: "-".join(map(str, k)))
def test_exact_tower_cases_meet_the_exactness_conditions(key):
    c = th.exact_tower_case(*key)
    seen = th.check_exact_tower(c, th.exact_tower_ref(*key))
    assert seen["top"] >= 8, "the case hardly leaves zero"
    if c.kind == "se":
        assert seen["gates"] == {0.5, 1.0}, "both gate values must occur"
    r32 = th.tower_ref(c, F32)                     # and the same formulas in float32 give the same numbers
    assert torch.equal(r32["x"].double(), th.exact_tower_ref(*key)["x"])


@pytest.mark.parametrize("key", th.STEM_CASES, ids=lambda k: "-".join(map(str, k)))
def test_stem_cases_meet_the_exactness_conditions(key):
    th.check_exact_stem(th.stem_case(*key))
    th.check_exact_stem(th.stem_case(*key, real=True), real=True)
    x = th.stem_ref(th.stem_case(*key, real=True), F64)["x"]       # every board: a constant plane and an all-zero plane
    assert torch.equal(x[:, :, 5].amin(1), x[:, :, 5].amax(1)) and float(x[:, :, 5].min()) > 0 and float(x[:, :, 9].max()) == 0


@pytest.mark.parametrize("key", th.TIER2_GP + th.TIER2_SE, ids=lambda k: "-".join(map(str, k)))
def test_tier2_cases_go_through_one_rounding(key):
    c = th.tier2_case(*key)
    th.check_single_rounding(c)
    r = th.tower_ref(c, F64)
    assert float(r["x"].max()) > 0.5
    if c.kind == "se2":
        x = r["x"]
        assert torch.equal(x[:, :, 5].amin(1), x[:, :, 5].amax(1)) and float(x[:, :, 5].min()) > 0 and float(x[:, :, 9].max()) == 0
        assert bool((x[:, :, 14].argmax(1) == 80).all()) and bool(((x[:, :, 14] == x[:, 80:, 14]).sum(1) == 1).all())
    # the judge passes the reference as a kernel would leave it, and has room for it: the stored value is inside the bound
    assert th.judge_x(th.qb(th.expect(c, F64)), c) <= 1.0
    assert all(v <= 1.0 for v in th.judge_pool(r["x"], th.stored_pool(r["pool"])).values())


# ------------------------------------------------------------------------------------------------ mutants


def exact_catches(mutant, keys):
    """the exact cases among `keys` on which the mutant reference differs from the reference in x_out or the max quarter"""
    hit = []
    for key in keys:
        c, ref = th.exact_tower_case(*key), th.exact_tower_ref(*key)
        m = th.tower_ref(c, F64, mutant=mutant)
        C = c.C
        if not (torch.equal(m["x"], ref["x"]) and torch.equal(m["pool"][:, C:2 * C], ref["pool"][:, C:2 * C])):
            hit.append(key)
    return hit


CONV3 = [k for k in th.EXACT_TOWER if k[0] == "conv" and k[6] == 3]
EXACT_MUTANTS = {
    "tap8_last_kstep": [k for k in th.EXACT_TOWER if k[0] == "conv"],
    "max_no_sq80": CONV3,
    "rot_not_bias": [k for k in th.EXACT_TOWER if k[0] == "conv" and k[4] == 5 and k[2] > 8],
    "prev_board_g": [k for k in th.EXACT_TOWER if k[0] == "conv" and k[4] == 5],
    "se_last_row": [k for k in th.EXACT_TOWER if k[0] == "se"],
    "se_halves_swapped": [k for k in th.EXACT_TOWER if k[0] == "se"],
    "next_model": [k for k in th.EXACT_TOWER if k[5] == 3],
}


@pytest.mark.parametrize("mutant", sorted(EXACT_MUTANTS))
def test_exact_tower_cases_catch_the_mutant(mutant):
    keys = EXACT_MUTANTS[mutant]
    hit = exact_catches(mutant, keys)
    if mutant == "max_no_sq80":                    # needs a channel whose maximum sits on square 80 alone: not in every case
        assert hit, mutant
    else:
        assert hit == keys, (mutant, [k for k in keys if k not in hit])


@pytest.mark.parametrize("mutant", ["rot_not_bias", "prev_board_g", "next_model", "se_last_row", "se_halves_swapped"])
def test_tier2_tower_cases_catch_the_mutant(mutant):
    keys = th.TIER2_SE if mutant.startswith("se_") else th.TIER2_GP + (th.TIER2_SE if mutant == "next_model" else ())
    if mutant == "rot_not_bias":
        keys = tuple(k for k in keys if k[2] > 8)  # (8 b) % 8 == 0: no rotation at G = 8
    for key in keys:
        c = th.tier2_case(*key)
        assert th.judge_x(th.qb(th.expect(c, F64, mutant)), c) > 1.0, (mutant, key)


@pytest.mark.parametrize("mutant", ["std_corr1", "max_no_sq80"])
def test_pooled_statistics_catch_the_mutant(mutant):
    name = {"std_corr1": "std", "max_no_sq80": "max"}[mutant]
    for key in th.TIER2_SE:
        x = th.tower_ref(th.tier2_case(*key), F64)["x"]
        pool = torch.cat([th.pool3(x, F64, mutant), torch.zeros(x.shape[0], x.shape[2], dtype=F64)], 1)
        assert th.judge_pool(x, th.stored_pool(pool))[name] > 1.0, (mutant, key)
    for key in th.STEM_CASES[:2] if mutant == "std_corr1" else ():
        x = th.stem_ref(th.stem_case(*key, real=True), F64)["x"]
        pool = torch.cat([th.pool3(x, F64, mutant), torch.zeros(x.shape[0], x.shape[2], dtype=F64)], 1)
        assert th.judge_pool(x, th.stored_pool(pool))["std"] > 1.0, (mutant, key)
    x = th.tower_ref(th.tier2_case(*th.TIER2_SE[0]), F64)["x"]
    pool = torch.cat([th.pool3(x, F64), torch.zeros(x.shape[0], x.shape[2], dtype=F64)], 1)
    tiny = pool.clone()
    tiny[0, 2 * x.shape[2] + 5] = 1e-7             # a constant plane whose std is not exactly 0
    assert th.judge_pool(x, tiny)["std"] == math.inf
    tiny = pool.clone()
    tiny[1, -1] = 1e-30
    assert th.judge_pool(x, tiny)["zero"] == math.inf


@pytest.mark.parametrize("mutant", ["stem_plane_cin", "next_model", "tap8_last_kstep"])
def test_stem_cases_catch_the_mutant(mutant):
    for key in th.STEM_CASES:
        C, cin, B, K = key
        if (mutant == "stem_plane_cin" and cin == 128) or (mutant == "next_model" and K == 1) or (mutant == "tap8_last_kstep" and cin <= 96):
            continue
        c = th.stem_case(*key)
        assert not torch.equal(th.stem_ref(c, F64, mutant=mutant)["x"], th.stem_ref(c, F64)["x"]), (mutant, key)
        c = th.stem_case(*key, real=True)
        got = th.stem_ref(c, F64, mutant=mutant)["x"]
        assert th.judge_x(got, c, lambda c, dt: th.stem_ref(c, dt)["pre"]) > 1.0, (mutant, key)


@pytest.mark.parametrize("mutant", ["move_major", "next_model"])
def test_heads_cases_catch_the_mutant(mutant):
    for key in th.HEADS_CASES:
        c = th.heads_case(*key)
        r = th.judge_heads({k: v.float() for k, v in th.heads_ref(c, F64, mutant).items()}, c)
        assert r["logits"] > 1.0, (mutant, key)
        if mutant == "next_model":
            assert r["value"] > 1.0 and r["score"] > 1.0, (mutant, key)
        ok = th.judge_heads({k: v.float() for k, v in th.heads_ref(c, F64).items()}, c)
        assert max(ok.values()) <= 1.0


def test_every_mutant_is_held_by_a_test():
    held = set(EXACT_MUTANTS) | {"std_corr1", "max_no_sq80", "stem_plane_cin", "move_major"}
    assert held == set(th.MUTANTS)
