"""CPU: the packed SL record (include/keisei_amd.h, KA_SL_PACKED_WORDS) in its numpy restatement ``pack_records`` /
``unpack_records`` -- the yardstick tests/test_hip_sl_device.py holds the kernels to.  Everything is a copy of bits, so
equality is exact."""
import numpy as np
import pytest

from keisei_amd.sl import prepare as prep
from keisei_amd.sl.dataset import NUM_ACTIONS, OBS_SIZE, RECORD_SIZE, SLDataset, _RECORD, write_shard
from keisei_amd.sl.device_dataset import PACKED_BYTES, PACKED_WORDS, pack_records, record_faults, unpack_records
from oracle import shogi as so
from sl_prepare_helpers import fixture_games

MAX_MOVES = 512


@pytest.fixture(scope="module")
def positions(golden):
    """The 784 positions of the fixture's 22 standard-start games, replayed through the oracle env (no game cut for its
    length: max_moves is prepare_sl_data's default)."""
    games, _ = fixture_games(golden("g15_sl_prepare"), MAX_MOVES)
    batch = prep.ReplayBatch.build(games)
    buf, valid_len, _, _ = prep._replay_host(batch, so.OracleVecEnv(batch.num_envs, MAX_MOVES))
    rec = buf[prep._kept_rows(batch, valid_len)].copy()
    rec.setflags(write=False)
    return rec


def crafted():
    """all-zero observation; a full plane of -0.0; only square 80; only squares 63 and 64 (the ballot boundary)."""
    rec = np.zeros(4, dtype=_RECORD)
    obs = rec["obs"].reshape(4, 50, 81)
    obs[1, 7, :] = -0.0
    obs[2, 49, 80] = 1.0
    obs[3, 13, 63] = obs[3, 13, 64] = 0.375
    rec["policy"], rec["value"], rec["score"] = [0, NUM_ACTIONS - 1, 17, 4000], [0, 1, 2, 1], [0.0, -0.5, 1.25, -0.0]
    return rec


def test_layout_constants():
    assert (PACKED_WORDS, PACKED_BYTES, PACKED_BYTES % 16) == (204, 816, 0)
    assert RECORD_SIZE == 16220 and OBS_SIZE == 4050


def test_fixture_positions_round_trip_byte_for_byte(positions):
    assert len(positions) == 784
    packed, first_bad = pack_records(positions)
    assert first_bad is None, f"position {first_bad} is reported as not packable"
    unpackable, bad_target = record_faults(positions)
    assert not unpackable.any() and not bad_target.any()
    assert packed.dtype == np.uint32 and packed.shape == (784, PACKED_WORDS)
    assert unpack_records(packed).tobytes() == positions.tobytes()
    # the words are what the header says they are, restated independently for one position with pieces in hand
    k = int(np.argmax((positions["obs"].reshape(-1, 50, 81)[:, 28:42] != 0).any(axis=(1, 2))))
    bits = positions["obs"][k].view(np.uint32).reshape(50, 81)
    for c in range(50):
        field = sum(1 << p for p in range(81) if bits[c, p])
        assert [int(w) for w in packed[k, 3 * c:3 * c + 3]] == [(field >> s) & 0xFFFFFFFF for s in (0, 32, 64)]
        assert int(packed[k, 150 + c]) == (int(bits[c][bits[c] != 0][0]) if field else 0)
    assert packed[k, 200:].tolist() == [int(positions["policy"][k]), int(positions["value"][k]),
                                        int(positions["score"][k:k + 1].view(np.uint32)[0]), 0]
    assert (packed[:, 203] == 0).all() and (packed[:, 2:150:3] >> 17 == 0).all()        # bits 81..95 stay zero


def test_crafted_records_round_trip():
    rec = crafted()
    packed, first_bad = pack_records(rec)
    assert first_bad is None
    assert unpack_records(packed).tobytes() == rec.tobytes()
    assert not packed[0, :200].any()
    # -0.0 is a non-zero pattern: the whole plane is set and its value is the sign bit
    assert packed[1, 21:24].tolist() == [0xFFFFFFFF, 0xFFFFFFFF, 0x1FFFF] and packed[1, 157] == 0x80000000
    assert packed[2, 147:150].tolist() == [0, 0, 1 << 16] and packed[2, 199] == np.float32(1.0).view(np.uint32)
    assert packed[3, 39:42].tolist() == [0, 1 << 31, 1] and packed[3, 163] == np.float32(0.375).view(np.uint32)


def test_unpackable_records_and_bad_targets_are_reported_with_their_index(positions, tmp_path):
    rec = np.concatenate([positions[:12], crafted()])
    two = 3
    rec["obs"].reshape(-1, 50, 81)[two, 44, [2, 70]] = [0.25, 0.5]              # two different non-zero values in one channel
    packed, first_bad = pack_records(rec)
    unpackable, bad_target = record_faults(rec)
    assert first_bad == two and np.nonzero(unpackable)[0].tolist() == [two] and not bad_target.any()
    for at, field, bad in ((5, "policy", NUM_ACTIONS), (6, "policy", -1), (9, "value", 3)):
        r = rec.copy()
        r["obs"][two] = positions["obs"][two]
        r[field][at] = bad
        _, first_bad = pack_records(r)
        unpackable, bad_target = record_faults(r)
        assert first_bad == at and np.nonzero(bad_target)[0].tolist() == [at] and not unpackable.any()
    # the lowest index wins whatever the kind
    r = rec.copy()
    r["value"][1] = -1
    assert pack_records(r)[1] == 1
    # the rule is SLDataset's: the same records in a shard raise there with the texts the device dataset repeats
    for field, bad, text in (("policy", NUM_ACTIONS, "Invalid policy_target=11259 at index 5 (shard=shard_0.bin, local=5): "
                                                       "must be in [0, 11259)"),
                             ("policy", -1, "Invalid policy_target=-1 at index 5"),
                             ("value", 3, "Invalid value_target=3 at index 5 (shard=shard_0.bin, local=5): "
                                          "must be 0 (W), 1 (D), or 2 (L)")):
        r = positions[:8].copy()
        r[field][5] = bad
        write_shard(tmp_path / "shard_0.bin", r["obs"], r["policy"], r["value"], r["score"])
        with pytest.raises(ValueError) as err:
            SLDataset(tmp_path)[5]
        assert text in str(err.value)
        assert record_faults(r)[1].tolist() == [False] * 5 + [True, False, False]


def test_device_resident_needs_the_fused_path(tmp_path):
    """On a CPU model either way of asking raises at construction; nothing falls back to the shard path."""
    from keisei_amd.sl.trainer import SLConfig, SLTrainer
    from keisei_amd.training.model_registry import build_model

    mp = dict(num_blocks=1, channels=32, se_reduction=8, global_pool_channels=16, policy_channels=8,
              value_fc_size=32, score_fc_size=16, obs_channels=50)
    assert SLConfig(data_dir=str(tmp_path)).device_resident is False
    assert list(SLConfig.__dataclass_fields__)[-1] == "device_resident"
    with pytest.raises(ValueError, match="fused HIP path"):
        SLTrainer(build_model("se_resnet", mp), SLConfig(data_dir=str(tmp_path), device_resident=True))
    trainer = SLTrainer(build_model("se_resnet", mp), SLConfig(data_dir=str(tmp_path)))
    assert trainer.device_dataset is None and trainer._order_override is None
