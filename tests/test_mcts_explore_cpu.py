"""The exploration of the visit-count search without a GPU: the controls and their table, the refusals, the C ABI, the float64
restatements of the root noise and of the drawn move (statistics and determinism), and the margin condition under which the
device tests of tests/test_hip_mcts_explore.py can hold the kernel to the restatement."""
import math
import re
from pathlib import Path

import numpy as np
import pytest

import mcts_explore_helpers as XH
from keisei_amd import _lib, build
from keisei_amd.training import MatchArena, MctsControls, MctsExploration, MctsStats, explore_table, root_noise_host, visit_choice_host
from keisei_amd.training import mcts_explore as X
from keisei_amd.training._device_ply import DevicePly
from keisei_amd.training.mcts_search import MctsStage
from keisei_amd.training.sampling import sample_uniform

ROOT = Path(__file__).resolve().parent.parent
ENVS = 4096


# ------------------------------------------------------------------ controls, table, refusals, ABI
def test_every_field_is_validated():
    c = MctsExploration(0.25, 0.15, 30)
    assert (c.noise_fraction, c.noise_alpha, c.sample_plies) == (0.25, 0.15, 30)
    assert MctsExploration() == MctsExploration(0.0, 0.0, 0) == MctsExploration.OFF
    MctsExploration(1.0, 0.01, 65535), MctsExploration(1, 100, 0), MctsExploration(0.0, 0.0, 5)
    for kw, msg in ((dict(noise_fraction=-0.1), r"noise_fraction must lie in \[0, 1\]"),
                    (dict(noise_fraction=1.5, noise_alpha=1.0), r"noise_fraction must lie in \[0, 1\]"),
                    (dict(noise_fraction=True), "noise_fraction must be a finite number"),
                    (dict(noise_fraction=float("nan")), "noise_fraction must be a finite number"),
                    (dict(noise_fraction="0.25"), "noise_fraction must be a finite number"),
                    (dict(noise_fraction=0.25), "noise_alpha must lie in"),
                    (dict(noise_fraction=0.25, noise_alpha=0.009), "noise_alpha must lie in"),
                    (dict(noise_fraction=0.25, noise_alpha=100.5), "noise_alpha must lie in"),
                    (dict(noise_fraction=0.25, noise_alpha=float("inf")), "noise_alpha must be a finite number"),
                    (dict(noise_fraction=0.25, noise_alpha=True), "noise_alpha must be a finite number"),
                    (dict(noise_alpha=-1.0), "noise_alpha must lie in"),
                    (dict(sample_plies=-1), "sample_plies must be an integer"),
                    (dict(sample_plies=65536), "sample_plies must be an integer"),
                    (dict(sample_plies=3.0), "sample_plies must be an integer"),
                    (dict(sample_plies=True), "sample_plies must be an integer")):
        with pytest.raises(ValueError, match=msg):
            MctsExploration(**kw)


def test_the_table_words_and_how_the_kernels_read_them():
    assert MctsExploration.OFF.row().tolist() == [0, 0, 0, 0]
    t = explore_table([MctsExploration(0.25, 0.15, 30), MctsExploration.OFF, MctsExploration(0.0, 0.0, 7)], 3)
    assert t.dtype == np.int32 and t.shape == (3, 4)
    assert t[:, :2].view(np.float32).tolist() == [[np.float32(0.25), np.float32(0.15)], [0.0, 0.0], [0.0, 0.0]]
    assert t[:, 2].tolist() == [30, 0, 7] and t[:, 3].tolist() == [0, 0, 0]
    assert not explore_table(None, 2).any() and np.array_equal(explore_table(MctsExploration(0.5, 1.0, 2), 2)[0],
                                                                explore_table(MctsExploration(0.5, 1.0, 2), 2)[1])
    eps, alpha, plies = X.explore_controls(t, [0, 1, 2, -1, 3])
    assert eps.tolist() == [0.25, 0, 0, 0, 0] and alpha.tolist() == [float(np.float32(0.15)), 0, 0, 0, 0]
    assert plies.tolist() == [30, 0, 7, 0, 0]
    # the bounds themselves are inside, as fp32
    edge = explore_table([MctsExploration(1.0, 0.01, 65535), MctsExploration(1.0, 100.0, 0)], 2)
    assert X.explore_controls(edge, [0, 1])[0].tolist() == [1.0, 1.0]
    # a row with a word out of range reads as OFF, whole
    f32 = lambda x: int(np.float32(x).view(np.int32))  # noqa: E731
    for col, word in ((0, f32(1.5)), (0, f32(-0.25)), (0, f32(float("nan"))), (1, f32(0.005)), (1, f32(101.0)),
                      (1, f32(float("nan"))), (2, -1), (2, 65536)):
        raw = t.copy()
        raw[0, col] = word
        assert [x.tolist()[0] for x in X.explore_controls(raw, [0])] == [0, 0, 0], (col, word)
    raw = t.copy()
    raw[2, 1] = f32(float("nan"))                             # alpha is not looked at when epsilon is 0
    assert X.explore_controls(raw, [2])[2].tolist() == [7]
    for bad, msg in ((([MctsExploration()] * 2, 3), "expected 3"), (([MctsControls(1)], 1), "must be a MctsExploration"),
                     ((MctsExploration(), 0), "at least one row"), (("x", 1), "mcts_explore must be None")):
        with pytest.raises(ValueError, match=msg):
            explore_table(*bad)


def test_the_refusals_need_no_device():
    on = MctsExploration(0.25, 0.15, 30)
    assert X.arena_mcts_explore(None, None, 2) is None and X.arena_mcts_explore(None, MctsControls(3, 4), 2) is None
    assert X.arena_mcts_explore(on, MctsControls(3, 4), 2).shape == (2, 4)
    with pytest.raises(ValueError, match="mcts_explore= needs mcts="):
        X.arena_mcts_explore(on, None, 2)
    with pytest.raises(ValueError, match="expected 2"):
        X.arena_mcts_explore([on], MctsControls(3, 4), 2)

    class Group:                                              # refused before anything touches a device
        device = None

        def __len__(self):
            return 2
    with pytest.raises(ValueError, match="mcts_explore= needs mcts="):
        MatchArena(Group(), 16, 8, 24, graph=False, mcts_explore=on)
    with pytest.raises(ValueError, match="an exploration needs mcts="):     # the stage that would own the table refuses
        DevicePly(Group(), 16, 24, stages=[MctsStage.parse(None, 2, False, explore_table(on, 2))])
    assert MctsStats() == MctsStats(0, 0, 0, 0, 0, 0) and MctsStats(1, 2, 3, 4, 5, 6) == MctsStats(1, 2, 3, 4, 5, 6, 0, 0, 0)
    assert (MctsStats().noised, MctsStats().sampled, MctsStats().diverged) == (0, 0, 0)


def test_the_abi_is_declared_exported_and_built():
    header = (ROOT / "include" / "keisei_amd.h").read_text()
    for name in ("ka_mcts_root_noise", "ka_mcts_advance_explore"):
        assert re.search(rf"\bint {name}\(", header) and name in _lib._SIGS and name in _lib.exported_symbols(), name
    assert len(_lib._SIGS["ka_mcts_advance_explore"].replace(" ", "")) == 23 + 5
    assert len(_lib._SIGS["ka_mcts_root_noise"].replace(" ", "")) == 11
    assert "mcts_explore.hip" in build.SOURCES and (ROOT / "keisei_amd" / "csrc" / "mcts_explore.hip").exists()
    assert _lib.query("ka_mcts_words", 7, 3, 4) == 4 and _lib.query("ka_mcts_words", 2, 3, 4) == 6
    # the stream constants stand in the header of the device code and in the module, and differ from the sampler's
    h = (ROOT / "keisei_amd" / "csrc" / "mcts_explore.h").read_text()
    assert f"0x{X.NOISE_STREAM:016X}ull" in h and f"0x{X.CHOICE_STREAM:016X}ull" in h
    assert len({X.NOISE_STREAM, X.CHOICE_STREAM, 0x5851F42D4C957F2D}) == 3


# ------------------------------------------------------------------ the noise: statistics
@pytest.mark.parametrize("alpha", [0.15, 1.0])
def test_gamma_and_dirichlet_moments(alpha):
    """Five standard errors from the distributions' own moments: Gamma(alpha) has mean and variance alpha; a symmetric
    Dirichlet's component has mean 1 / n and variance (1 / n)(1 - 1 / n) / (n alpha + 1)."""
    n, seed = 8, 20261021
    a32 = float(np.float32(alpha))                            # alpha as the table holds it
    g = np.array([X.dirichlet_gammas_host(seed, e, n, a32)[0] for e in range(ENVS)])
    assert g.shape == (ENVS, n) and (g >= 0).all()
    assert abs(g.mean() - alpha) <= 5 * math.sqrt(alpha / g.size)
    priors = np.full((ENVS, n), 0.125, np.float32)
    _, eta, margin = root_noise_host(seed, priors, np.full(ENVS, n), np.ones(ENVS, bool), MctsExploration(0.25, alpha, 0), None)
    np.testing.assert_allclose(eta, g / g.sum(1, keepdims=True), rtol=1e-14)
    np.testing.assert_allclose(eta.sum(1), 1.0, rtol=1e-12)
    se = math.sqrt((1 / n) * (1 - 1 / n) / (n * alpha + 1) / ENVS)
    assert (np.abs(eta.mean(0) - 1 / n) <= 5 * se).all(), (eta.mean(0), se)
    assert np.isfinite(margin).all() and (margin > 0).all()


def test_the_prior_mass_is_kept_and_off_is_the_identity():
    rng = np.random.default_rng(5)
    B, W = 512, 8
    p = rng.random((B, W))
    p = (p / (p.sum(1, keepdims=True) * rng.uniform(1.0, 2.0, (B, 1)))).astype(np.float32)
    n_cand = rng.integers(1, W + 1, B)
    active = rng.random(B) < 0.9
    model_of = rng.integers(-1, 3, B)                         # model 2 lies outside the table
    ctl = [MctsExploration(0.25, 0.15, 0), MctsExploration(0.0, 0.0, 9)]
    out, eta, margin = root_noise_host(77, p, n_cand, active, ctl, model_of)
    noised = active & (model_of == 0)
    assert out.dtype == np.float32 and noised.sum() > 50
    assert np.array_equal(out[~noised].view(np.int32), p[~noised].view(np.int32)) and not eta[~noised].any()
    assert np.isinf(margin[~noised]).all() and np.isfinite(margin[noised]).all()
    changed = 0
    for b in np.flatnonzero(noised):
        n = int(n_cand[b])
        assert np.array_equal(out[b, n:].view(np.int32), p[b, n:].view(np.int32)) and not eta[b, n:].any()
        s0, s1 = float(p[b, :n].astype(np.float64).sum()), float(out[b, :n].astype(np.float64).sum())
        assert abs(s1 - s0) <= 1e-6 * s0, b               # fp32 rounding of at most 8 terms
        if n == 1:
            assert out[b, 0] == p[b, 0] and eta[b, 0] == 1.0
        changed += int((out[b, :n] != p[b, :n]).any())
    assert changed > 40
    # epsilon 0 returns the priors to the bit, whatever alpha and sample_plies say
    same, eta0, _ = root_noise_host(77, p, n_cand, active, MctsExploration(0.0, 0.5, 30), None)
    assert np.array_equal(same.view(np.int32), p.view(np.int32)) and not eta0.any()


# ------------------------------------------------------------------ the noise: determinism
def test_the_draws_are_a_function_of_seed_and_env():
    p = np.full((8, 8), 0.1, np.float32)
    args = (np.full(8, 8), np.ones(8, bool), MctsExploration(0.25, 0.15, 0), None)
    a, eta_a, _ = root_noise_host(123, p, *args)
    b, eta_b, _ = root_noise_host(123, p, *args)
    c, eta_c, _ = root_noise_host(124, p, *args)
    assert np.array_equal(a.view(np.int32), b.view(np.int32)) and np.array_equal(eta_a.view(np.int64), eta_b.view(np.int64))
    assert len({eta_a[e].tobytes() for e in range(8)}) == 8                      # another env, other bits
    assert all(eta_a[e].tobytes() != eta_c[e].tobytes() for e in range(8))       # another seed, other bits
    # the noise stream, the choice stream and the sampler's uniform of one (seed, env) are three different draws
    for seed, env in ((123, 0), (123, 5), (2 ** 62 + 11, 4095)):
        h_n, h_c = X.noise_stream(seed, env), X.noise_stream(seed, env, X.CHOICE_STREAM)
        assert h_n != h_c
        u = {X.draw_uniform(X.stream_draw(h_n, 0)), X.draw_uniform(X.stream_draw(h_c, 0)), sample_uniform(seed, env)}
        assert len(u) == 3 and all(0.0 < x < 1.0 for x in u)
        assert h_n >> 40 != int(sample_uniform(seed, env) * 16777216)            # nor is it the sampler's stream itself
    assert X.draw_uniform(0) == 2.0 ** -53 and X.draw_uniform(2 ** 64 - 1) == 1.0 - 2.0 ** -53


# ------------------------------------------------------------------ the choice
def test_the_move_is_drawn_in_proportion_to_the_visits():
    visits = np.tile(np.array([5, 3, 0, 8]), (ENVS, 1))
    ctl = [MctsExploration(0.0, 0.0, 10), MctsExploration(0.0, 0.0, 3)]
    slot, sampled = visit_choice_host(99, visits, np.full(ENVS, 4), np.full(ENVS, 9), ctl, np.zeros(ENVS, np.int64))
    assert sampled.all() and not (slot == 2).any()
    for k, n_k in enumerate((5, 3, 0, 8)):
        q = n_k / 16
        assert abs((slot == k).mean() - q) <= 5 * math.sqrt(q * (1 - q) / ENVS), k
    # at and behind sample_plies the first arg-max is played, and a model off or outside the table never draws
    for ply, model in ((10, 0), (11, 0), (3, 1), (9, 1), (0, -1), (0, 2)):
        slot, sampled = visit_choice_host(99, visits[:64], np.full(64, 4), np.full(64, ply), ctl, np.full(64, model))
        assert (slot == 3).all() and not sampled.any(), (ply, model)
    slot, sampled = visit_choice_host(99, [[4, 7, 7, 1]], [4], [50], ctl, [0])
    assert slot.tolist() == [1] and not sampled.any()         # ties keep the lower slot
    slot, sampled = visit_choice_host(99, [[4, 7, 9, 1]] * 64, [2] * 64, [0] * 64, ctl, [0] * 64)
    assert sampled.all() and set(slot.tolist()) == {0, 1}     # only the n_cand slots count
    a = visit_choice_host(99, visits[:64], np.full(64, 4), np.zeros(64), ctl, None)[0]
    b = visit_choice_host(100, visits[:64], np.full(64, 4), np.zeros(64), ctl, None)[0]
    assert not np.array_equal(a, b) and np.array_equal(a, visit_choice_host(99, visits[:64], np.full(64, 4), np.zeros(64), ctl, None)[0])


# ------------------------------------------------------------------ the margin condition of the device tests
@pytest.mark.parametrize("W", XH.NOISE_W)
def test_no_test_of_the_device_cases_is_decided_by_less_than_the_margin(W):
    """The device's fp64 log / cos / exp differ from the host's by a few units in 1e-16: with every accept test and every
    sign test of the fixed seeds decided by at least 1e-9, no branch of the draw can differ on the device."""
    for B in XH.NOISE_B:
        c = XH.noise_case(B, W)
        _, _, margin = root_noise_host(c["seed"], c["priors"], c["n_cand"], c["active"], c["ctl"], c["model_of"])
        noised = c["active"] & (c["model_of"] == 0)
        assert noised[0] and np.isfinite(margin[noised]).all() and np.isinf(margin[~noised]).all()
        assert (margin >= XH.MARGIN).all(), (B, W, float(margin.min()))
        if B >= 7:
            assert (~c["active"]).any() and (c["model_of"] == 1).any() and (c["model_of"] == -1).any()
        if B >= 9:
            assert set(c["n_cand"].tolist()) == set(range(1, W + 1))


def test_nor_is_one_of_the_real_env_step():
    for n in range(1, XH.STEP_W + 1):
        for e in range(XH.STEP_ENVS):
            assert X.dirichlet_gammas_host(XH.STEP_SEED, e, n, float(np.float32(XH.STEP_ALPHA)))[1] >= XH.MARGIN, (n, e)


def test_the_shared_table_reader_and_field_checks():
    from test_lookahead_cpu import check_field_refusals, check_table_of
    check_table_of(explore_table, "mcts_explore", MctsExploration(0.25, 0.15, 30), [MctsExploration(0.5, 1.0, 2), MctsExploration()])
    check_field_refusals(MctsExploration, ints=(("sample_plies", 65535),))
