"""CPU: the left-right reflection of SL positions in its numpy restatement (``mirror_action`` / ``mirror_records`` /
``sl_mirror_draw`` of keisei_amd.sl.device_dataset) -- the yardstick tests/test_hip_sl_mirror.py holds ``ka_sl_gather_aug``
to -- against the CPU rules oracle: two envs in lockstep, one on a position and one on its file-reversed image, must show
reflected observations, permuted legal masks and identical outcomes at every position.  Equality is exact throughout."""
from pathlib import Path

import numpy as np
import pytest

from keisei_amd import _lib
from keisei_amd.sl import device_dataset as dd
from keisei_amd.sl import prepare as prep
from keisei_amd.sl.dataset import NUM_ACTIONS, OBS_SIZE, _RECORD
from keisei_amd.sl.device_dataset import (mirror_action, mirror_records, pack_records, sl_mirror_draw, unpack_records)
from oracle import shogi as so
from sl_prepare_helpers import fixture_games

M64 = 2 ** 64 - 1
GPU_TEST_SEEDS = (0, 20260, -3, 2 ** 64 - 1)         # the seeds tests/test_hip_sl_mirror.py draws with


# ---------------------------------------------------------------------------------------------- the action table
def test_mirror_action_is_a_permutation_and_an_involution():
    a = np.arange(NUM_ACTIONS)
    m = mirror_action(a)
    assert m.dtype == np.int64 and sorted(m.tolist()) == a.tolist()
    assert np.array_equal(mirror_action(m), a)
    assert (m // 139 // 9 == a // 139 // 9).all() and (m // 139 % 9 == 8 - a // 139 % 9).all()
    assert mirror_action(np.zeros((2, 0, 3), np.int64)).shape == (2, 0, 3)
    for bad in (-1, NUM_ACTIONS):
        with pytest.raises(ValueError, match="action indices"):
            mirror_action([0, bad])


def test_mirror_action_against_a_hand_written_table():
    """One slot of each kind at square (3, 2) -> (3, 6).  Directions clockwise from north: N NE E SE S SW W NW = 0..7."""
    N, NE, E, SE, S, SW, W, NW = range(8)
    frm, to = (3 * 9 + 2) * 139, (3 * 9 + 6) * 139
    table = []
    for promote in (0, 64):
        for dist, (d, md) in enumerate(((N, N), (NE, NW), (E, W), (SE, SW), (S, S), (SW, SE), (W, E), (NW, NE))):
            table.append((frm + promote + d * 8 + dist % 8, to + promote + md * 8 + dist % 8))
    table += [(frm + 128, to + 130), (frm + 129, to + 131), (frm + 130, to + 128), (frm + 131, to + 129)]      # both knights
    table += [(frm + 132 + 4, to + 132 + 4), (frm + 138, to + 138)]                                          # drops
    table += [(0, 8 * 139), (4 * 139 + 7, 4 * 139 + 7), (NUM_ACTIONS - 1, 72 * 139 + 138)]      # corners, the centre file
    got = mirror_action([a for a, _ in table]).tolist()
    assert got == [b for _, b in table]


def test_mirror_action_agrees_with_the_oracle_decoder():
    """Every index the oracle decodes as a move on the board, for both colours: the reflected index decodes to the move
    with both files reversed (the white perspective 80 - q commutes with the reflection)."""
    def flip(q):
        return q - q % 9 + 8 - q % 9

    seen = 0
    for white in (False, True):
        for a in range(0, NUM_ACTIONS, 7):
            mv = so.decode(a, white=white)
            if mv is None:
                continue
            frm, to, promote, drop = mv
            want = (frm if drop else flip(frm), flip(to), promote, drop)
            assert so.decode(int(mirror_action(a)), white=white) == want, (a, white)
            seen += 1
    assert seen > 1000


# ---------------------------------------------------------------------------------------------- against the rules
def flip_board(board):
    return np.ascontiguousarray(np.asarray(board).reshape(9, 9)[:, ::-1]).reshape(81)


def make_records(obs, actions):
    rec = np.zeros(len(actions), dtype=_RECORD)
    rec["obs"] = obs.reshape(len(actions), OBS_SIZE)
    rec["policy"] = actions
    rec["value"] = np.arange(len(actions)) % 3
    rec["score"] = np.linspace(-1.0, 1.0, len(actions), dtype=np.float32)
    return rec


def test_lockstep_oracle_envs_on_a_position_and_its_reflection():
    E, MAX_PLY, STEPS = 8, 60, 600
    rng = np.random.default_rng(2026)
    left, right = so.OracleVecEnv(E, MAX_PLY), so.OracleVecEnv(E, MAX_PLY)
    obs_l, mask_l = left.reset()
    obs_r, mask_r = right.reset()
    perm = mirror_action(np.arange(NUM_ACTIONS))

    def seat(e):
        """Both envs seated by set_state, the right one on the file-reversed image (the standard start is not its own
        image: rook and bishop change sides), so that ply and history agree."""
        board, hands, side, _ = left.state(e)
        left.set_state(e, board, hands, side)
        right.set_state(e, flip_board(board), hands, side)
        obs_l[e], mask_l[e] = left.observe(e)
        obs_r[e], mask_r[e] = right.observe(e)

    for e in range(E):
        seat(e)
    positions = finished = 0
    keys = ("rewards", "terminated", "truncated", "termination_reason", "ply_count", "material_balance", "captured_piece",
            "current_players")
    for _ in range(STEPS):
        # the position: all 50 planes and the legal mask, no env left out
        assert np.array_equal(obs_r, obs_l[:, :, :, ::-1])
        assert np.array_equal(mask_r[:, perm], mask_l)
        acts = np.array([rng.choice(np.nonzero(mask_l[e])[0]) for e in range(E)], dtype=np.int64)
        macts = mirror_action(acts)
        # the record: mirror_records of (obs, action) is the record built from the reflected env, byte for byte
        assert mirror_records(make_records(obs_l, acts)).tobytes() == make_records(obs_r, macts).tobytes()
        positions += E
        out_l, out_r = left.step(acts), right.step(macts)
        for k in keys:
            assert np.array_equal(out_l[k], out_r[k]), k
        done = out_l["terminated"] | out_l["truncated"]
        assert np.array_equal(out_r["terminal_observations"][done], out_l["terminal_observations"][done][:, :, :, ::-1])
        obs_l, mask_l, obs_r, mask_r = (out_l["observations"], out_l["legal_masks"], out_r["observations"],
                                        out_r["legal_masks"])
        for e in np.nonzero(done)[0]:
            seat(int(e))                                         # a finished game restarted from the standard start
            finished += 1
    assert positions == 4800 and finished >= 40
    print(f"{positions} positions, {finished} finished games")


# ---------------------------------------------------------------------------------------------- the packed record
@pytest.fixture(scope="module")
def positions(golden):
    games, _ = fixture_games(golden("g15_sl_prepare"), 512)
    batch = prep.ReplayBatch.build(games)
    buf, valid_len, _, _ = prep._replay_host(batch, so.OracleVecEnv(batch.num_envs, 512))
    rec = buf[prep._kept_rows(batch, valid_len)].copy()
    rec.setflags(write=False)
    return rec


def reflected_decode(packed) -> np.ndarray:
    """What ``ka_sl_gather_aug`` does in mode 1, from the header's text: bit r * 9 + (8 - f) where the plain decode reads
    bit r * 9 + f, the policy through the closed form."""
    pk = np.asarray(packed, dtype=np.uint32)
    n = len(pk)
    rec = np.zeros(n, dtype=_RECORD)
    obs = np.zeros((n, 50, 81), dtype=np.uint32)
    for p in range(81):
        q = p - p % 9 + 8 - p % 9
        bit = (pk[:, np.arange(50) * 3 + (q >> 5)] >> np.uint32(q & 31)) & np.uint32(1)
        obs[:, :, p] = np.where(bit == 1, pk[:, 150:200], 0)
    rec["obs"] = obs.reshape(n, OBS_SIZE).view(np.float32)
    rec["policy"] = mirror_action(pk[:, 200].view(np.int32).astype(np.int64))
    rec["value"] = pk[:, 201].view(np.int32)
    rec["score"] = pk[:, 202].view(np.float32)
    return rec


def test_packing_commutes_with_the_reflection_on_the_fixture_positions(positions):
    assert len(positions) == 784
    packed, first_bad = pack_records(positions)
    assert first_bad is None
    mirrored = mirror_records(positions)
    mpacked, first_bad = pack_records(mirrored)
    assert first_bad is None
    assert unpack_records(mpacked).tobytes() == mirrored.tobytes() == reflected_decode(packed).tobytes()
    assert mirror_records(mirrored).tobytes() == positions.tobytes()
    assert (mirrored["policy"] != positions["policy"]).any() and (mirrored["obs"] != positions["obs"]).any()
    assert np.array_equal(mirrored["value"], positions["value"]) and np.array_equal(mirrored["score"], positions["score"])
    with pytest.raises(TypeError, match="shard record dtype"):
        mirror_records(np.zeros(3))


# ---------------------------------------------------------------------------------------------- the draw
def mix_int(x: int) -> int:
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def draw_int(seed: int, epoch: int, i: int) -> bool:
    h = mix_int((seed & M64) ^ mix_int((((epoch << 32) | (i & 0xFFFFFFFF)) + 0x6D6972726F72) & M64))
    return bool(h >> 63)


def test_mirror_draw_against_python_integers():
    idx = np.concatenate([np.arange(784), [2 ** 31 - 1, 2 ** 20, 123456789]])
    for seed in GPU_TEST_SEEDS:
        for epoch in (0, 1, 2, 2 ** 31 - 1):
            got = sl_mirror_draw(seed, epoch, idx)
            assert got.dtype == bool and got.shape == idx.shape
            assert got.tolist() == [draw_int(seed, epoch, int(i)) for i in idx], (seed, epoch)
            assert got[:784].any() and not got[:784].all(), (seed, epoch)         # both outcomes occur
        assert not np.array_equal(sl_mirror_draw(seed, 0, idx), sl_mirror_draw(seed, 1, idx))
    assert not np.array_equal(sl_mirror_draw(0, 0, idx), sl_mirror_draw(1, 0, idx))
    # a function of (seed, epoch, position) alone: any order, any shape
    order = np.random.default_rng(0).permutation(784)
    assert np.array_equal(sl_mirror_draw(7, 3, order.reshape(28, 28)), sl_mirror_draw(7, 3, np.arange(784))[order].reshape(28, 28))
    share = sl_mirror_draw(11, 0, np.arange(100000)).mean()
    assert 0.49 < share < 0.51, share
    with pytest.raises(ValueError, match="epoch"):
        sl_mirror_draw(0, -1, idx)


# ---------------------------------------------------------------------------------------------- plumbing
def test_entry_points_are_bound_declared_and_exported():
    names = set(_lib.exported_symbols())
    header = (Path(__file__).resolve().parent.parent / "include" / "keisei_amd.h").read_text()
    for n in ("ka_sl_gather_aug", "ka_sl_eval"):
        assert n in names and f"int {n}(" in header, n
    assert _lib._SIGS["ka_sl_gather_aug"].replace(" ", "") == _lib._SIGS["ka_sl_gather"].replace(" ", "")[:-1] + "iqip"
    assert "0x6D6972726F72" in header
    for n in ("mirror_action", "mirror_records", "sl_mirror_draw"):
        assert n in dd.__all__ and callable(getattr(dd, n)), n
    assert (dd.MIRROR_NONE, dd.MIRROR_ALL, dd.MIRROR_DRAWN) == (0, 1, 2)


def test_trainer_configuration(tmp_path):
    from keisei_amd.sl.trainer import SLConfig, SLTrainer
    from keisei_amd.training.model_registry import build_model

    mp = dict(num_blocks=1, channels=32, se_reduction=8, global_pool_channels=16, policy_channels=8,
              value_fc_size=32, score_fc_size=16, obs_channels=50)
    cfg = SLConfig(data_dir=str(tmp_path))
    assert cfg.mirror_augment is False and cfg.mirror_seed == 0
    # the positional order of the reference's fields and of device_resident is untouched
    assert SLConfig(str(tmp_path), 64, 1e-3, 3, 0, 1.0, 1.5, 0.02, 0.5, False, False, True).device_resident is True
    with pytest.raises(ValueError, match="mirror_seed"):
        SLConfig(data_dir=str(tmp_path), mirror_seed=2 ** 64)
    with pytest.raises(ValueError, match="mirror_augment"):                       # the shard path cannot reflect
        SLTrainer(build_model("se_resnet", mp), SLConfig(data_dir=str(tmp_path), mirror_augment=True))
    with pytest.raises(ValueError, match="fused HIP path"):                       # and a CPU model has no device path
        SLTrainer(build_model("se_resnet", mp), SLConfig(data_dir=str(tmp_path), mirror_augment=True, device_resident=True))
    trainer = SLTrainer(build_model("se_resnet", mp), SLConfig(data_dir=str(tmp_path)))
    assert trainer.eval_dataset is None and trainer.epochs_done == 0
    with pytest.raises(ValueError, match="needs a dataset"):
        trainer.evaluate()
    trainer.train_epoch()
    assert trainer.epochs_done == 1
