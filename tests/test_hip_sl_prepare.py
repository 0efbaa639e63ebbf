"""GPU: SL shard preparation on the device (csrc/sl_prepare.hip behind keisei_amd.sl.prepare) against its host restatement
``_replay_host`` over the CPU env oracle, byte for byte, and against tests/golden/g15_*.  Exact equality throughout."""
import json
import math

import numpy as np
import pytest
import torch

from keisei_amd.sl import prepare as prep
from keisei_amd.sl.dataset import OBS_SIZE, RECORD_SIZE, SLDataset
from keisei_amd.sl.parsers import is_standard_start
from oracle import shogi as so
from sl_prepare_helpers import FILES, GOLDEN, check_against_golden, fixture_games, parsed_records

pytestmark = pytest.mark.gpu
ENVS, GUARD = 64, 3
MP = dict(num_blocks=1, channels=32, se_reduction=8, global_pool_channels=16, policy_channels=8,
          value_fc_size=32, score_fc_size=16, obs_channels=50)


@pytest.fixture(scope="module")
def device_replay(golden):
    return prep._DeviceReplay(ENVS, int(golden("g15_sl_prepare").np("max_moves")))


def replay_guarded(dev, batch):
    """The batch on the device into a buffer with GUARD rows of 0xA5 in front and behind; the whole buffer comes back."""
    buf = torch.full(((batch.rows + 2 * GUARD) * RECORD_SIZE,), 0xA5, dtype=torch.uint8, device=dev.device)
    out = buf[GUARD * RECORD_SIZE:(GUARD + batch.rows) * RECORD_SIZE]
    none, valid_len, reason, hdr = dev.replay(batch, out=out)
    assert none is None
    return buf.cpu().numpy().reshape(-1, RECORD_SIZE), valid_len, reason, hdr


@pytest.mark.parametrize("num_games", [3, 64, 130])
def test_kernels_equal_the_host_restatement_byte_for_byte(golden, device_replay, num_games):
    g = golden("g15_sl_prepare")
    max_moves = int(g.np("max_moves"))
    games, _ = fixture_games(g, repeat=6)
    games = games[:num_games]
    sizes, parities = [], set()
    for chunk in prep._batches(games, ENVS, 10 ** 9):
        batch = prep.ReplayBatch.build(chunk)
        sizes.append(len(chunk))
        parities |= {int(r) & 1 for r, n in zip(batch.row_of, batch.length) if n}
        raw, valid_len, reason, hdr = replay_guarded(device_replay, batch)
        padded = batch.padded(ENVS)
        want, want_len, want_reason, want_hdr = prep._replay_host(padded, so.OracleVecEnv(ENVS, max_moves))
        assert np.array_equal(valid_len, want_len) and np.array_equal(reason, want_reason)
        assert hdr[:6].tolist() == want_hdr[:6].tolist() and hdr[6:].tolist() == [0, 0]
        assert (raw[:GUARD] == 0xA5).all() and (raw[-GUARD:] == 0xA5).all(), "a sentinel row was written"
        body = raw[GUARD:-GUARD]
        kept = prep._kept_rows(padded, valid_len)
        assert (body[~kept] == 0xA5).all(), "the row of a cut move was written"
        assert kept.sum() == hdr[prep._WRITTEN]
        mism = np.nonzero((body != want.view(np.uint8).reshape(-1, RECORD_SIZE)).any(axis=1))[0]
        assert mism.size == 0, f"rows {mism[:8].tolist()} differ from the host restatement"
    assert sizes == {3: [3], 64: [64], 130: [64, 64, 2]}[num_games]
    assert parities == {0, 1}                                    # rows at 8-byte aligned and at merely 4-byte aligned offsets


def test_device_records_equal_the_golden_and_a_plain_oracle_replay(golden, device_replay):
    g = golden("g15_sl_prepare")
    max_moves = int(g.np("max_moves"))
    games, index = fixture_games(g)
    batch = prep.ReplayBatch.build(games)
    buf, valid_len, reason, hdr = device_replay.replay(batch)
    buf, n = buf.copy(), len(games)
    padded = batch.padded(ENVS)
    # every kept record against the fixture: policy, value, material / 76, observation checksum, valid_len and reasons
    raw = buf.view(np.uint8).reshape(-1, RECORD_SIZE).copy()
    raw[~prep._kept_rows(padded, valid_len)] = 0xA5               # (the replay's own buffer has no sentinel fill)
    check_against_golden(g, games, index, batch, raw.reshape(-1).view(buf.dtype), valid_len[:n], reason[:n])
    # observations bit for bit against one-game-at-a-time oracle replays of the kept moves
    for e in range(n):
        env = so.OracleVecEnv(1, max_moves)
        obs, _ = env.reset()
        rows = buf[int(batch.row_of[e]):int(batch.row_of[e]) + int(valid_len[e])]
        for rec in rows:
            assert np.array_equal(rec["obs"].view(np.uint32), obs.reshape(-1).view(np.uint32))
            obs = env.step([int(rec["policy"])])["observations"]
    # counters
    assert int(hdr[prep._ILLEGAL]) == int((g.np("reason") == 1).sum())
    assert int(hdr[prep._RULES]) == int(g.np("games_cut_by_rules")) and int(hdr[prep._WRITTEN]) == len(g.np("pos_policy"))
    assert int(hdr[prep._PLIES]) == int(batch.length.max()) and int(hdr[prep._WRITTEN] + hdr[prep._FILLER]) == ENVS * int(hdr[prep._PLIES])


def test_prepare_sl_data_counters_equal_the_golden(golden, tmp_path):
    g = golden("g15_sl_prepare")
    meta = prep.prepare_sl_data([str(GOLDEN)], str(tmp_path), min_ply=1, shard_size=100, batch_envs=ENVS,
                                max_moves=int(g.np("max_moves")))
    n = len(g.np("pos_policy"))
    assert meta == {"placeholder": False, "num_shards": (n + 99) // 100, "num_games": int(g.np("standard_start").sum()),
                    "num_positions": n, "games_cut_illegal": int(g.np("games_cut_illegal")),
                    "games_cut_by_rules": int(g.np("games_cut_by_rules")), "games_cut_long": int(g.np("games_cut_long")),
                    "games_nonstandard_start": int(g.np("games_nonstandard_start"))}
    got = SLDataset(tmp_path).read_batch(np.arange(n))
    order = np.argsort(g.np("pos_game"), kind="stable")          # the fixture lists positions game by game, in record order
    assert np.array_equal(order, np.arange(n))
    assert np.array_equal(got["policy_target"].numpy(), g.np("pos_policy"))
    assert np.array_equal(got["value_target"].numpy(), g.np("pos_value"))
    assert np.array_equal(got["score_target"].numpy(), g.np("pos_material").astype(np.float32) / np.float32(76.0))


def test_prepare_sl_data_files_equal_the_host_restatement(golden, tmp_path):
    """shard_size = 7, max_moves = 20: shards, metadata and SLDataset.read_batch against ``_replay_host``; a second run
    with fewer games leaves no stale shard; the directory trains."""
    g = golden("g15_sl_prepare")
    max_moves = 20
    out = tmp_path / "shards"
    meta = prep.prepare_sl_data([str(f) for f in FILES], str(out), min_ply=1, shard_size=7, batch_envs=8, max_moves=max_moves,
                                max_batch_positions=100)
    games, _ = fixture_games(g, max_moves)
    want_parts, final = [], []
    for chunk in prep._batches(games, 8, 100):                   # the host restatement, batch by batch
        batch = prep.ReplayBatch.build(chunk)
        buf, valid_len, reason, _ = prep._replay_host(batch, so.OracleVecEnv(batch.num_envs, max_moves))
        want_parts.append(buf[prep._kept_rows(batch, valid_len)])
        final += np.where(reason != 0, reason, np.array([x[2] for x in chunk])[batch.order]).tolist()
    want = np.concatenate(want_parts)
    n, final = len(want), np.array(final)
    shards = sorted(out.glob("shard_*.bin"))
    assert [s.name for s in shards] == [f"shard_{k:03d}.bin" for k in range((n + 6) // 7)]
    assert b"".join(s.read_bytes() for s in shards) == want.tobytes()
    assert all(s.stat().st_size == 7 * RECORD_SIZE for s in shards[:-1])
    assert json.loads((out / "shard_meta.json").read_text()) == meta
    assert meta == {"placeholder": False, "num_shards": len(shards), "num_games": len(games), "num_positions": n,
                    "games_cut_illegal": int(((final == 1) | (final == 4)).sum()), "games_cut_by_rules": int((final == 2).sum()),
                    "games_cut_long": sum(len(r.moves) > max_moves for r in parsed_records() if is_standard_start(r.start)),
                    "games_nonstandard_start": int(g.np("games_nonstandard_start"))}
    ds = SLDataset(out)
    got = ds.read_batch(np.arange(n))
    assert torch.equal(got["observation"].reshape(n, OBS_SIZE), torch.from_numpy(want["obs"].copy()))
    assert torch.equal(got["policy_target"], torch.from_numpy(want["policy"].copy()))
    assert torch.equal(got["value_target"], torch.from_numpy(want["value"].copy()))
    assert torch.equal(got["score_target"], torch.from_numpy(want["score"].copy()))

    # the produced directory trains (a smoke check, not parity)
    from keisei_amd.sl.trainer import SLConfig, SLTrainer
    from keisei_amd.training.model_registry import build_model
    torch.manual_seed(15)
    trainer = SLTrainer(build_model("se_resnet", MP).to("cuda"), SLConfig(data_dir=str(out), batch_size=n, total_epochs=2))   # one step
    met = trainer.train_epoch()
    assert met and all(math.isfinite(v) for v in met.values()), met

    # a second run into the same directory with fewer games
    meta2 = prep.prepare_sl_data([str(FILES[0])], str(out), min_ply=30, shard_size=7, batch_envs=8, max_moves=max_moves,
                                 max_batch_positions=100)
    assert 0 < meta2["num_games"] < meta["num_games"] and meta2["num_shards"] < meta["num_shards"]
    assert len(list(out.glob("shard_*.bin"))) == meta2["num_shards"] and len(SLDataset(out)) == meta2["num_positions"]
