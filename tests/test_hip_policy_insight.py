"""ka_policy_insight on the GPU against the float64 numpy restatement of the reference's showcase lines
(policy_insight_helpers.oracle_row: runner.py:151-173, heatmap.py:40-49).  Every case uses the whole spatial action space
(11 259 actions): 5 crafted rows and 67 seeded rows.  Probabilities, entropy and win probability carry the project's fp32
output tolerance (rtol 1e-4 / atol 5e-5); actions, ranks, counts, flags and the candidate order are exact.  For bf16
logits the oracle gets the same bf16-rounded values."""
import numpy as np
import pytest
import torch

from keisei_amd import _lib
from keisei_amd.shogi_gym import ACTION_SPACE, MASK_WORDS
from keisei_amd.training import policy_insight
from keisei_amd.training.policy_insight import HEAT_WORDS, insight_words
from policy_insight_helpers import ATOL, RTOL, as_numpy, check_rows, crafted_rows, oracle_of, seeded_rows

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = 0x5A5A5A5A


def _stream():
    return _lib.stream_ptr(torch.device(DEV))


def _pack(legal) -> torch.Tensor:
    masks = torch.as_tensor(legal).to(DEV).contiguous()
    bits = torch.zeros(masks.shape[0], MASK_WORDS, dtype=torch.int32, device=DEV)
    _lib.call("ka_pack_mask_bits", masks, bits, masks.shape[0], ACTION_SPACE, _stream())
    return bits


def _launch(logits, bits, actions, *, vlogits=None, players=None, model_of=None, K=1, temperature=1.0, top_k=3, spare=0,
            hist_len=0, count=None):
    """One raw launch into sentinel-filled buffers of B + spare rows; returns (last, heat, hist, flags) on the host."""
    B, W = logits.shape[0], insight_words(top_k)
    full = lambda *s: torch.full(s, SENTINEL, dtype=torch.int32, device=DEV)  # noqa: E731
    last, heat = full(B + spare, W), full(B + spare, HEAT_WORDS)
    hist = full(B + spare, hist_len, W) if hist_len else None
    flags = torch.zeros(2, dtype=torch.int32, device=DEV)
    _lib.call("ka_policy_insight", logits, int(logits.dtype == torch.bfloat16), bits, MASK_WORDS, actions, vlogits, players,
              model_of, K, temperature, top_k, last, heat.view(torch.float32), hist, hist_len, count, flags, B, ACTION_SPACE,
              _stream())
    return last.cpu().numpy(), heat.cpu().numpy(), None if hist is None else hist.cpu().numpy(), flags.cpu().numpy()


def _device_rows(which, bf16):
    logits, legal, actions, vlogits, players = crafted_rows() if which == "crafted" else seeded_rows()
    lg = torch.from_numpy(logits).to(DEV)
    if bf16:
        lg = lg.to(torch.bfloat16)
    return lg, legal, torch.from_numpy(actions).to(DEV), torch.from_numpy(vlogits).to(DEV), torch.from_numpy(players).to(DEV)


@pytest.mark.parametrize("top_k", [1, 3, 8])
@pytest.mark.parametrize("temperature", [1.0, 0.5])
@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("which", ["crafted", "seeded"])
def test_kernel_matches_the_oracle(which, bf16, temperature, top_k):
    lg, legal, actions, vlogits, players = _device_rows(which, bf16)
    packed = top_k != 3                                       # bool rows and packed rows both reach the kernel
    lm = _pack(legal) if packed else torch.from_numpy(legal).to(DEV)
    res = as_numpy(policy_insight(lg, lm, actions, vlogits, players=players, temperature=temperature, top_k=top_k))
    check_rows(res, oracle_of(which, bf16, temperature), top_k, which)
    assert ((res["flags"] >> 1) & 1).tolist() == players.tolist() and not int(res["nan_flag"][0])
    assert res["records"][:, 1].tolist() == np.clip(actions.cpu().numpy(), -1, ACTION_SPACE).tolist()
    if which == "crafted":                                    # one legal move: fewer candidates than top_k are padded
        assert res["top_actions"][0].tolist() == [int(actions[0])] + [-1] * (top_k - 1)
        assert res["top_probabilities"][0].tolist() == [1.0] + [0.0] * (top_k - 1)
        assert res["chosen_probability"][0] == 1.0 and res["entropy"][0] == 0.0 and res["chosen_rank"][0] == 0
        if top_k == 8:
            assert res["top_actions"][4][:4].tolist() == [17, 4242, 9000, 11258]       # bitwise-equal logits: lower action first


def test_device_and_host_paths_agree():
    lg, legal, actions, vlogits, players = _device_rows("seeded", False)
    dev = as_numpy(policy_insight(lg, torch.from_numpy(legal).to(DEV), actions, vlogits, players=players, temperature=0.5, top_k=8))
    host = as_numpy(policy_insight(lg.cpu(), torch.from_numpy(legal), actions.cpu(), vlogits.cpu(), players=players.cpu(),
                                   temperature=0.5, top_k=8))
    for key in ("n_legal", "chosen_rank", "flags", "top_actions"):
        assert np.array_equal(dev[key], host[key]), key
    for key in ("chosen_probability", "entropy", "win_probability", "top_probabilities", "heat"):
        np.testing.assert_allclose(dev[key], host[key], rtol=RTOL, atol=ATOL, err_msg=key)


def test_invalid_rows_are_zero_records():
    lg, legal, actions, vlogits, players = _device_rows("crafted", False)
    legal = legal.copy()
    legal[1] = False                                          # no legal action
    model_of = torch.tensor([0, 0, -1, 1, 0], dtype=torch.int32, device=DEV)    # rows 2 and 3: outside [0, 1)
    last, heat, _, flags = _launch(lg, _pack(legal), actions, vlogits=vlogits, players=players, model_of=model_of, K=1)
    assert not last[1:4].any() and not heat[1:4].any()        # zeros over the sentinel, n_legal 0 among them
    assert last[0, 0] & 1 and last[4, 0] & 1 and last[0, 2] == 1 and last[4, 2] == 10
    assert flags.tolist() == [0, 0]
    want = oracle_of("crafted", False, 1.0)
    np.testing.assert_allclose(last[4].view(np.float32)[4], want[4]["chosen_probability"], rtol=RTOL, atol=ATOL)


def test_nan_flag_follows_legal_logits_only():
    lg, legal, actions, vlogits, _ = _device_rows("crafted", False)
    bits = _pack(legal)
    lg = lg.clone()
    lg[2, 1] = float("nan")                                   # row 2: action 1 is not legal
    assert _launch(lg, bits, actions)[3].tolist() == [0, 0]
    lg[2, 3] = float("nan")                                   # action 3 is
    assert _launch(lg, bits, actions)[3].tolist() == [1, 0]


def test_chosen_probability_is_the_samplers():
    """At temperature 1 the insight shows the distribution the sampler draws from: p[action] = exp(log-prob)."""
    lg, legal, _, _, _ = _device_rows("seeded", False)
    B, bits = lg.shape[0], _pack(legal)
    act = torch.empty(B, dtype=torch.int64, device=DEV)
    lp = torch.empty(B, device=DEV)
    nl = torch.empty(B, dtype=torch.int32, device=DEV)
    sflags = torch.zeros(2, dtype=torch.int32, device=DEV)
    model_of = torch.zeros(B, dtype=torch.int32, device=DEV)
    _lib.call("ka_policy_sample_play", lg, 0, bits, MASK_WORDS, torch.tensor([20261019], dtype=torch.int64, device=DEV),
              model_of, 1, act, lp, nl, sflags, B, ACTION_SPACE, _stream())
    res = as_numpy(policy_insight(lg, bits, act, model_of=model_of, num_models=1, temperature=1.0, top_k=1))
    assert np.array_equal(res["n_legal"], nl.cpu().numpy()) and (res["flags"] & 4).all()
    np.testing.assert_allclose(res["chosen_probability"], np.exp(lp.cpu().numpy().astype(np.float64)), rtol=RTOL, atol=ATOL)


@pytest.mark.parametrize("top_k", [1, 8])
def test_guard_band_stays_intact(top_k):
    lg, legal, actions, vlogits, players = _device_rows("seeded", False)
    B, row_len = lg.shape[0], 4
    count = (torch.arange(B + 1, dtype=torch.int32) % (row_len + 2)).to(DEV)      # 0 .. row_len + 1: some rows write nothing
    last, heat, hist, _ = _launch(lg, _pack(legal), actions, vlogits=vlogits, players=players, top_k=top_k, spare=1,
                                  hist_len=row_len, count=count)
    s = np.int32(SENTINEL)
    assert (last[B] == s).all() and (heat[B] == s).all() and (hist[B] == s).all()
    assert not (last[:B] == s).all(axis=1).any()


def test_history_slot_is_the_move_count():
    lg, legal, actions, vlogits, players = _device_rows("crafted", False)
    row_len = 5
    count = torch.tensor([0, 3, row_len, 4, -1], dtype=torch.int32, device=DEV)
    last, _, hist, _ = _launch(lg, _pack(legal), actions, vlogits=vlogits, players=players, hist_len=row_len, count=count)
    s = np.int32(SENTINEL)
    for b, c in enumerate([0, 3, None, 4, None]):
        for slot in range(row_len):
            if slot == c:
                assert np.array_equal(hist[b, slot], last[b]), (b, slot)
            else:
                assert (hist[b, slot] == s).all(), (b, slot)


def test_arguments_are_refused():
    lg, legal, actions, _, _ = _device_rows("crafted", False)
    bits = _pack(legal)
    for kw, msg in (({"top_k": 0}, "top_k"), ({"top_k": 9}, "top_k"), ({"temperature": 0.0}, "temperature"),
                    ({"temperature": -1.0}, "temperature")):
        with pytest.raises((_lib.KeiseiHipError, ValueError), match=msg):
            _launch(lg, bits, actions, **kw)
    B = lg.shape[0]
    buf = torch.zeros(B, insight_words(3), dtype=torch.int32, device=DEV)
    heat = torch.zeros(B, HEAT_WORDS, device=DEV)
    flags = torch.zeros(2, dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.KeiseiHipError, match="spatial action space"):
        _lib.call("ka_policy_insight", lg, 0, bits, MASK_WORDS, actions, None, None, None, 1, 1.0, 3, buf, heat, None, 0, None,
                  flags, B, 13527, _stream())
    hist = torch.zeros(B, 2, insight_words(3), dtype=torch.int32, device=DEV)
    with pytest.raises(_lib.KeiseiHipError, match="row_len"):
        _lib.call("ka_policy_insight", lg, 0, bits, MASK_WORDS, actions, None, None, None, 1, 1.0, 3, buf, heat, hist, 0,
                  torch.zeros(B, dtype=torch.int32, device=DEV), flags, B, ACTION_SPACE, _stream())
