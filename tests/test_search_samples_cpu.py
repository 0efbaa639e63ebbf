"""CPU: the search-sample store's restatement ``search_sample_step_host`` on a hand-written script of plies (every expected
word comes from the script's own tables in tests/search_samples_helpers.py), the visit-word format, the numpy restatements
of the visit gather, the float64 reference of ``ka_policy_ce_soft`` against torch's cross-entropy, and the refusals of the
new options."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import search_samples_helpers as S
import update_head_helpers as H
from keisei_amd import _lib
from keisei_amd.sl import device_dataset as dd
from keisei_amd.sl.dataset import NUM_ACTIONS
from keisei_amd.sl.trainer import SLConfig, SLTrainer
from keisei_amd.training import search_samples as ss
from keisei_amd.training.mcts_search import MctsControls

ROOT = Path(__file__).resolve().parent.parent
NEW = ("ka_search_sample_step", "ka_search_sample_words", "ka_sl_gather_visits", "ka_policy_ce_soft")


def test_symbols_in_header_and_binding_table():
    header = (ROOT / "include" / "keisei_amd.h").read_text()
    for name in NEW:
        assert re.search(rf"\bint {name}\(", header), name
        assert name in _lib.exported_symbols()
    sig = lambda n: len(_lib._SIGS[n].replace(" ", ""))  # noqa: E731
    assert (sig("ka_search_sample_step"), sig("ka_sl_gather_visits"), sig("ka_policy_ce_soft")) == (19, 11, 12)
    assert "#define KA_SEARCH_SAMPLE_WORDS 216" in header and "#define KA_SL_VISIT_WORDS 8" in header
    assert (ss.ROW_WORDS, ss.ROW_BYTES, ss.META_WORDS, dd.VISIT_SLOTS, dd.INFO_WORDS) == (216, 864, 5, 8, 4)
    assert "search_samples.hip" in __import__("keisei_amd.build", fromlist=["SOURCES"]).SOURCES
    if _lib.available():
        assert [_lib.query("ka_search_sample_words", i) for i in range(6)] == [216, 5, 8, 4, 1 << 20, -1]


# ------------------------------------------------------------------------------------------------ refusals
class _Group:
    """Enough of a group for MatchArena's argument checks, which come before anything touches a device."""
    device = torch.device("cpu")
    _tables = None

    def __len__(self):
        return 2


def test_search_samples_needs_mcts():
    from keisei_amd.training.match_arena import MatchArena
    with pytest.raises(ValueError, match="search_samples needs mcts="):
        MatchArena(_Group(), 8, 4, 16, graph=False, search_samples=4)
    with pytest.raises(ValueError, match="search_samples needs mcts="):
        MatchArena(_Group(), 8, 4, 16, graph=False, search_samples=4, mcts=MctsControls())        # every width 0
    with pytest.raises(ValueError, match="non-negative integer"):
        MatchArena(_Group(), 8, 4, 16, graph=False, search_samples=-1, mcts=MctsControls(width=3, simulations=4))
    with pytest.raises(ValueError, match="GPU group"):          # with mcts= the option passes; the CPU group is refused next
        MatchArena(_Group(), 8, 4, 16, graph=False, search_samples=4, mcts=MctsControls(width=3, simulations=4))


def test_visit_targets_needs_a_device_dataset(tmp_path):
    cfg = SLConfig(str(tmp_path), 8, visit_targets=True)
    assert cfg.visit_targets and not cfg.device_resident and SLConfig(str(tmp_path)).visit_targets is False
    assert SLConfig("d", 8, 1e-3, 30, 0, 1.0, 1.5, 0.02, 0.5, False, False, True).device_resident       # the last positional
    model = torch.nn.Linear(2, 2)
    model.configure_amp = lambda **kw: None
    with pytest.raises(ValueError, match="visit_targets trains on the visit rows"):
        SLTrainer(model, cfg)


def _bare_dataset(n: int, with_visits: bool):
    """A DeviceSLDataset without a device: the mixing checks come before anything is launched."""
    ds = object.__new__(dd.DeviceSLDataset)
    ds._device, ds._n, ds._read_only, ds._unread = torch.device("cpu"), n, False, []
    ds._packed = torch.zeros(n, dd.PACKED_WORDS, dtype=torch.int32)
    ds._visits = torch.zeros(n, 8, dtype=torch.int32) if with_visits else None
    ds._info = torch.zeros(n, 4, dtype=torch.int32) if with_visits else None
    return ds


def test_append_packed_refuses_to_mix():
    packed, visits = torch.zeros(2, 204, dtype=torch.int32), torch.zeros(2, 8, dtype=torch.int32)
    with pytest.raises(ValueError, match="without visit rows"):
        _bare_dataset(3, False).append_packed(packed, visits)
    with pytest.raises(ValueError, match="holds visit rows"):
        _bare_dataset(3, True).append_packed(packed)
    with pytest.raises(ValueError, match="holds visit rows"):
        _bare_dataset(3, True).append_raw(torch.zeros(16220, dtype=torch.uint8), [0])
    with pytest.raises(ValueError, match="needs visits="):
        _bare_dataset(0, False).append_packed(packed, None, torch.zeros(2, 4, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"visits must be a contiguous int32 tensor \(2, 8\)"):
        _bare_dataset(3, True).append_packed(packed, torch.zeros(2, 7, dtype=torch.int32))
    with pytest.raises(ValueError, match="needs a dataset with visit rows"):
        _bare_dataset(3, False).gather(torch.zeros(1, dtype=torch.int64), torch.zeros(1, dtype=torch.int32), visit_targets=True)
    ds = _bare_dataset(3, True)
    assert ds.visits.shape == (3, 8) and ds.info.shape == (3, 4) and _bare_dataset(3, False).visits is None


# ------------------------------------------------------------------------------------------------ the word format
def test_visit_words_round_trip():
    a = np.array([[11258, 7, 0], [5, 6, 7]])
    v = np.array([[64, 0, 1], [0, 0, 0]])
    w = ss.visit_words(a, v)
    assert w.dtype == np.uint32 and w.shape == (2, 8)
    assert w[0].tolist() == [11258 | (64 << 16), 0, 1 << 16, 0, 0, 0, 0, 0] and not w[1].any()
    acts, vis = ss.unpack_visit_words(w)
    assert acts[0].tolist() == [11258, -1, 0, -1, -1, -1, -1, -1] and vis[0].tolist() == [64, 0, 1, 0, 0, 0, 0, 0]
    assert (acts[1] == -1).all() and not vis[1].any()
    g = np.random.default_rng(0)
    a, v = g.integers(0, NUM_ACTIONS, (50, 8)), g.integers(0, 65, (50, 8))
    acts, vis = ss.unpack_visit_words(ss.visit_words(a, v))
    assert np.array_equal(vis, v) and np.array_equal(acts, np.where(v > 0, a, -1))
    with pytest.raises(ValueError):
        ss.visit_words([NUM_ACTIONS], [1])
    with pytest.raises(ValueError):
        ss.visit_words(np.zeros(9, int), np.ones(9, int))


def test_visit_weights():
    g = np.random.default_rng(1)
    v = g.integers(0, 65, (200, 8))
    v[0], v[1] = 0, (64, 0, 0, 0, 0, 0, 0, 0)
    words = ss.visit_words(g.integers(0, NUM_ACTIONS, v.shape), v)
    w = dd.visit_weights(words)
    assert w.dtype == np.float32 and not w[0].any() and w[1].tolist() == [1.0] + [0.0] * 7
    total = v.sum(1, keepdims=True)
    exact = np.divide(v, total, out=np.zeros(v.shape), where=total > 0)
    assert np.abs(w - exact).max() <= 2.0 ** -24                         # one rounding of a quotient in [0, 1]
    with np.errstate(invalid="ignore"):
        one = np.where(v > 0, v.astype(np.float32) / total.astype(np.float32), np.float32(0))
    assert np.array_equal(w.view(np.uint32), one.astype(np.float32).view(np.uint32))
    assert np.abs(w.sum(1)[1:].astype(np.float64) - 1.0).max() < 1e-6


def test_mirror_visit_words():
    g = np.random.default_rng(2)
    a, v = g.integers(0, NUM_ACTIONS, (300, 8)), g.integers(0, 4, (300, 8))
    words = ss.visit_words(a, v)
    m = dd.mirror_visit_words(words)
    assert m.dtype == np.uint32 and np.array_equal(dd.mirror_visit_words(m), words)
    acts, vis = ss.unpack_visit_words(m)
    assert np.array_equal(vis, v)
    assert np.array_equal(acts, np.where(v > 0, dd.mirror_action(a), -1))
    assert np.array_equal(m[v == 0], words[v == 0]) and (m != words).any()


# ------------------------------------------------------------------------------------------------ the loss reference
@pytest.mark.parametrize("A", (1, 33, 257))
@pytest.mark.parametrize("K", (1, 8))
def test_soft_ce_reference_is_the_cross_entropy_on_dense_targets(A, K):
    logits, actions, weights = S.soft_case(A, K)
    w_policy = 1.0 / S.SOFT_B
    ref = S.soft_ce_ref(logits, actions, weights, w_policy, torch.float64)
    lg = logits.double().requires_grad_(True)
    rows = F.cross_entropy(lg, S.dense_targets(actions, weights, A), reduction="none")
    (dl,) = torch.autograd.grad(w_policy * rows.sum(), lg)
    assert torch.allclose(ref["rowloss"], rows.detach(), rtol=0, atol=1e-12)
    assert torch.allclose(ref["dlogits"], dl, rtol=0, atol=1e-12)


@pytest.mark.parametrize("A", (1, 33, 11259))
def test_soft_ce_reference_one_hot_is_policy_ce_ref(A):
    case = H.policy_case(A, 3)
    actions = case.actions[case.idx].to(torch.int32)[:, None]
    for dt in (torch.float64, torch.float32):
        ref = S.soft_ce_ref(case.logits, actions, torch.ones(H.PB, 1), H.W.lambda_policy / H.PB, dt)
        old = H.policy_ce_ref(case, dt)
        assert torch.equal(ref["rowloss"], old["rowloss"]) and torch.equal(ref["dlogits"], old["dlogits"])


# ------------------------------------------------------------------------------------------------ the script
@pytest.mark.parametrize("W", (3, 8))
def test_step_host_on_the_script(W):
    rows, meta = np.zeros((S.E, S.R, ss.ROW_WORDS), np.uint32), np.zeros((S.E, ss.META_WORDS), np.int32)
    for t in range(S.T):
        p = S.script_ply(t, W)
        err = ss.search_sample_step_host(rows, meta, p["obs"], p["players"], p["records"], p["root_visits"], p["model_of"],
                                         p["actions"], p["material"], p["rewards"], p["terminated"], p["truncated"])
        assert err == 0
        for (e, at), want in S.META_AT.items():
            if at == t:
                assert tuple(meta[e]) == want, (e, t)
    want_rows, want_meta = S.expected_store(W)
    assert np.array_equal(meta, want_meta), meta
    for e in range(S.E):
        for r in range(S.R):
            bad = np.flatnonzero(rows[e, r] != want_rows[e, r])
            assert bad.size == 0, (e, r, bad, rows[e, r, bad], want_rows[e, r, bad])
    # spot values, as literals: env 0's row 2 was written at ply 2 with all 8 (or 3) candidates, its score is 38 / 76
    assert rows[0, 2, 202] == 0x3F000000 and rows[0, 2, 204] == (201 | (3 << 16)) and rows[0, 2, 201] == 0
    assert rows[0, 2, 204 + W - 1] == (200 + W) | ((1 + (2 + W - 1) % 5) << 16) and (W == 8 or rows[0, 2, 207] == 0)
    assert rows[3, 2, 201] == 0xFFFFFFFF and rows[3, 2, 212] == 1 and rows[3, 0, 212] == (1 | (1 << 16))
    assert rows[1, 2, 200] == 1000 + 34 + 1 and not rows[4, 2].any()
    assert rows[4, 0, 205] == (42 | (1 << 16)) and rows[4, 0, 206] == 0          # n_cand 2: the stale third count is not written


def test_step_host_flags_an_unpackable_observation():
    rows, meta = np.zeros((S.E, S.R, ss.ROW_WORDS), np.uint32), np.zeros((S.E, ss.META_WORDS), np.int32)
    p = S.script_ply(0, 3)
    p["obs"][3, 81 * 7 + 4], p["obs"][3, 81 * 7 + 9] = 1.0, 2.0             # env 3 is inactive at ply 0: never packed
    args = lambda: (p["obs"], p["players"], p["records"], p["root_visits"], p["model_of"], p["actions"], p["material"],  # noqa: E731
                    p["rewards"], p["terminated"], p["truncated"])
    assert ss.search_sample_step_host(rows, meta, *args()) == 0
    p["obs"][1, 81 * 7 + 4], p["obs"][1, 81 * 7 + 9] = 1.0, 2.0
    assert ss.search_sample_step_host(rows, meta, *args()) == ss.ERR_UNPACKABLE


def test_random_script_keeps_the_invariants():
    script = S.random_script(5)
    rows, meta = np.zeros((S.E, S.R, ss.ROW_WORDS), np.uint32), np.zeros((S.E, ss.META_WORDS), np.int32)
    wants = np.zeros(S.E, int)
    for t in range(len(script[0])):
        p = S.script_ply(t, 8, script)
        ss.search_sample_step_host(rows, meta, p["obs"], p["players"], p["records"], p["root_visits"], p["model_of"],
                                   p["actions"], p["material"], p["rewards"], p["terminated"], p["truncated"])
        wants += np.array([a and min(n, 8) >= 1 and m >= 0 for a, n, m, *_ in (script[e][t] for e in range(S.E))])
    assert np.array_equal(meta[:, 0] + meta[:, 2], wants) and (meta[:, 0] <= S.R).all() and (meta[:, 1] <= meta[:, 0]).all()
    assert meta[:, 2].any() and meta[:, 4].any()
    for e in range(S.E):
        values = rows[e, :, 201].view(np.int32)
        assert (values[:meta[e, 1]] >= 0).all() and (values[:meta[e, 1]] <= 2).all() and (values[meta[e, 1]:meta[e, 0]] == -1).all()
