"""GPU: the packed, device-resident SL dataset (csrc/sl_data.hip behind keisei_amd.sl.device_dataset) against its numpy
restatement ``pack_records`` / ``unpack_records`` and against ``SLDataset``, and the device-resident epoch of ``SLTrainer``
against the shard epoch.  Everything up to the trainer is a copy of bits: equality is exact."""
import json

import numpy as np
import pytest
import torch

from keisei_amd import _lib
from keisei_amd.sl import DeviceSLDataset, prepare_sl_dataset
from keisei_amd.sl import prepare as prep
from keisei_amd.sl.dataset import OBS_SIZE, RECORD_SIZE, SLDataset, _RECORD
from keisei_amd.sl.device_dataset import PACKED_BYTES, PACKED_WORDS, pack_records, record_faults, unpack_records
from keisei_amd.sl.trainer import SLConfig, SLTrainer
from keisei_amd.training.model_registry import build_model
from oracle import shogi as so
from sl_prepare_helpers import FILES, fixture_games

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAX_MOVES = 512
INT_MAX = 2 ** 31 - 1
GUARD = 0xA5
MP = dict(num_blocks=2, channels=32, se_reduction=8, global_pool_channels=16, policy_channels=8,
          value_fc_size=32, score_fc_size=16, obs_channels=50)


@pytest.fixture(scope="module")
def positions(golden):
    """The 784 positions of the fixture's standard-start games through the CPU oracle env, and their packed rows."""
    games, _ = fixture_games(golden("g15_sl_prepare"), MAX_MOVES)
    batch = prep.ReplayBatch.build(games)
    buf, valid_len, _, _ = prep._replay_host(batch, so.OracleVecEnv(batch.num_envs, MAX_MOVES))
    rec = buf[prep._kept_rows(batch, valid_len)].copy()
    assert len(rec) == 784
    packed, first_bad = pack_records(rec)
    assert first_bad is None
    rec.setflags(write=False)
    packed.setflags(write=False)
    return rec, packed


@pytest.fixture(scope="module")
def shard_dir(positions, tmp_path_factory):
    """The positions as three shards of 300, 300 and 184 records."""
    rec, _ = positions
    out = tmp_path_factory.mktemp("sl_device_shards")
    for k, (lo, hi) in enumerate(((0, 300), (300, 600), (600, 784))):
        rec[lo:hi].tofile(out / f"shard_{k}.bin")
    return out


def to_device(records) -> torch.Tensor:
    return torch.from_numpy(np.frombuffer(records.tobytes(), dtype=np.uint8).copy()).to(DEV)


def guarded(nbytes: int, pad: int = 816):
    """A device byte buffer of ``nbytes`` between two guards of 0xA5 bytes: ``(whole, body)``."""
    whole = torch.full((nbytes + 2 * pad,), GUARD, dtype=torch.uint8, device=DEV)
    return whole, whole[pad:pad + nbytes]


def guards_intact(whole: torch.Tensor, nbytes: int, pad: int = 816) -> bool:
    host = whole.cpu().numpy()
    return bool((host[:pad] == GUARD).all() and (host[pad + nbytes:] == GUARD).all())


def run_pack(records, src_rows, n):
    raw = to_device(records)
    whole, body = guarded(n * PACKED_BYTES)
    flags = torch.tensor([0, INT_MAX, 0, INT_MAX], dtype=torch.int32, device=DEV)
    rows = None if src_rows is None else torch.from_numpy(np.asarray(src_rows, dtype=np.int64)).to(DEV)
    _lib.call("ka_sl_pack", raw, rows, n, body, flags, _lib.stream_ptr())
    assert guards_intact(whole, n * PACKED_BYTES), "ka_sl_pack wrote outside its rows"
    return body.cpu().numpy().view(np.uint32).reshape(n, PACKED_WORDS), flags.cpu().tolist()


# ---------------------------------------------------------------------------------------------- the two kernels
def test_library_and_module_agree_on_the_packed_record():
    assert _lib.query("ka_sl_packed_words") == PACKED_WORDS == 204


@pytest.mark.parametrize("n", [1, 63, 64, 65, 784])
def test_pack_kernel_equals_pack_records(positions, n):
    rec, want = positions
    got, flags = run_pack(rec[:n], None, n)                      # null src_rows: row i
    assert np.array_equal(got, want[:n]) and flags == [0, INT_MAX, 0, INT_MAX]
    src = (np.arange(n) * 5 + 1) % 784                           # skips rows; odd and even rows (8- and 4-byte aligned)
    assert n == 1 or {int(r) & 1 for r in src} == {0, 1}
    got, flags = run_pack(rec, src, n)
    assert np.array_equal(got, want[src]) and flags == [0, INT_MAX, 0, INT_MAX]


def test_pack_kernel_crafted_planes_and_flags(positions):
    rec, _ = positions
    r = rec[:64].copy()
    obs = r["obs"].reshape(64, 50, 81)
    obs[1] = 0.0                                                 # an all-zero observation
    obs[2, 7, :] = -0.0                                          # a full plane of -0.0
    obs[3, 49, :], obs[3, 49, 80] = 0.0, 1.0                     # only square 80
    obs[4, 13, :], obs[4, 13, 63:65] = 0.0, 0.375                # only squares 63 and 64: the ballot boundary
    want, first_bad = pack_records(r)
    assert first_bad is None
    got, flags = run_pack(r, None, 64)
    assert np.array_equal(got, want) and flags == [0, INT_MAX, 0, INT_MAX]
    assert unpack_records(got).tobytes() == r.tobytes()
    # records 5 and 9 cannot be packed, record 7 has a bad target: exact counts and lowest indices
    obs[9, 44, [2, 70]] = [0.25, 0.5]
    obs[5, 3, 80] = 2.0
    obs[5, 3, 0] = 1.0
    r["policy"][7] = 11259
    unpackable, bad_target = record_faults(r)
    assert np.nonzero(unpackable)[0].tolist() == [5, 9] and np.nonzero(bad_target)[0].tolist() == [7]
    got, flags = run_pack(r, None, 64)
    assert flags == [2, 5, 1, 7]
    ok = ~(unpackable | bad_target)
    assert np.array_equal(got[ok], pack_records(r)[0][ok])
    for field, bad in (("policy", -1), ("value", 3), ("value", -1), ("policy", 2 ** 32 + 5)):
        r2 = rec[:8].copy()
        r2[field][6] = bad
        assert run_pack(r2, None, 8)[1] == [0, INT_MAX, 1, 6], (field, bad)


def run_gather(packed, n, idx):
    B = len(idx)
    pk = torch.from_numpy(np.array(packed).view(np.int32)).to(DEV)
    sizes = (B * OBS_SIZE * 4, B * 8, B * 8, B * 4)
    bufs = [guarded(s, pad=16) for s in sizes]
    obs = bufs[0][1].view(torch.float32).view(B, 50, 9, 9)
    policy, value = bufs[1][1].view(torch.int64), bufs[2][1].view(torch.int64)
    score = bufs[3][1].view(torch.float32)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    _lib.call("ka_sl_gather", pk, n, torch.tensor(idx, dtype=torch.int64, device=DEV), B, obs, policy, value, score, flag,
              _lib.stream_ptr())
    for (whole, _), s in zip(bufs, sizes):
        assert guards_intact(whole, s, pad=16), "ka_sl_gather wrote outside an output"
    got = np.zeros(B, dtype=_RECORD)
    got["obs"] = obs.cpu().numpy().reshape(B, OBS_SIZE)
    got["policy"], got["value"], got["score"] = policy.cpu().numpy(), value.cpu().numpy(), score.cpu().numpy()
    return got, int(flag.item())


@pytest.mark.parametrize("B", [1, 3, 257])
def test_gather_kernel_equals_unpack_records(positions, B):
    rec, packed = positions
    n = len(rec)
    rng = np.random.default_rng(B)
    idx = {1: [n - 1], 3: [0, n - 1, 0]}.get(B)
    if idx is None:
        idx = rng.integers(0, 40, B).tolist()                    # 257 draws from 40 rows: repeats
        idx[5], idx[200], idx[256] = 0, n - 1, n - 1
        idx[6:150] = rng.integers(0, n, 144).tolist()
    got, flag = run_gather(packed, n, idx)
    assert flag == 0
    assert got.tobytes() == unpack_records(packed[idx]).tobytes() == rec[idx].tobytes()


def test_gather_kernel_flags_an_index_outside_the_dataset(positions):
    rec, packed = positions
    n = len(rec)
    idx = [3, n, 0, n - 1, -1, 3, 17]
    got, flag = run_gather(packed, n, idx)
    assert flag == 2
    want = rec[[3, 0, 0, n - 1, 0, 3, 17]].copy()
    want[[1, 4]] = np.zeros(2, dtype=_RECORD)                    # zero observation, targets of 0
    assert got.tobytes() == want.tobytes()
    # a dataset shorter than its allocation: rows past n are outside
    got, flag = run_gather(packed, 10, [9, 10])
    assert flag == 1 and got[:1].tobytes() == rec[9:10].tobytes() and got[1:].tobytes() == bytes(RECORD_SIZE)


# ---------------------------------------------------------------------------------------------- the dataset
def test_from_shards_equals_sldataset(positions, shard_dir):
    rec, packed = positions
    ds = DeviceSLDataset.from_shards(shard_dir, chunk_records=128)          # 300 = 2 * 128 + 44: chunks straddle files
    assert len(ds) == 784 and ds.nbytes == 784 * 816 and ds.device.type == "cuda"
    assert np.array_equal(ds.packed.cpu().numpy().view(np.uint32), packed)
    i = np.random.default_rng(3).permutation(784)
    got, want = ds.read_batch(i), SLDataset(shard_dir).read_batch(i)
    assert got.keys() == want.keys()
    for k in want:
        assert got[k].device.type == "cuda" and got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, k
        assert got[k].cpu().numpy().tobytes() == want[k].numpy().tobytes(), k
    for bad in ([0, 784], [-1]):
        with pytest.raises(IndexError, match=f"index {bad[-1]} out of range for dataset with 784 positions"):
            ds.read_batch(bad)
    whole = DeviceSLDataset.from_shards(shard_dir)              # the default chunk is larger than the dataset
    assert np.array_equal(whole.packed.cpu().numpy().view(np.uint32), packed)


def test_from_shards_refusals(positions, shard_dir, tmp_path, monkeypatch):
    rec, _ = positions

    def write(records, meta=None):
        for old in tmp_path.glob("shard_*"):
            old.unlink()
        for k, (lo, hi) in enumerate(((0, 300), (300, 600), (600, 784))):
            records[lo:hi].tofile(tmp_path / f"shard_{k}.bin")
        if meta is not None:
            (tmp_path / "shard_meta.json").write_text(json.dumps(meta))

    write(rec, {"placeholder": True})
    with pytest.raises(ValueError, match="placeholder"):
        DeviceSLDataset.from_shards(tmp_path, chunk_records=128)
    assert len(DeviceSLDataset.from_shards(tmp_path, chunk_records=128, allow_placeholder=True)) == 784

    for field, bad in (("policy", 11259), ("value", 3)):
        r = rec.copy()
        r[field][317] = bad
        r[field][650] = bad                                      # the lowest index is the one reported
        write(r)
        with pytest.raises(ValueError) as want:
            SLDataset(tmp_path)[317]
        assert "index 317 (shard=shard_1.bin, local=17)" in str(want.value)
        with pytest.raises(ValueError) as got:
            DeviceSLDataset.from_shards(tmp_path, chunk_records=128)
        assert str(got.value) == str(want.value)

    r = rec.copy()
    r["obs"].reshape(-1, 50, 81)[617, 44, [2, 70]] = [0.25, 0.5]
    write(r)
    with pytest.raises(ValueError) as got:
        DeviceSLDataset.from_shards(tmp_path, chunk_records=128)
    assert "index 617 (shard=shard_2.bin, local=17): channel values are not one-valued planes; this dataset cannot be " \
           "held packed" in str(got.value)

    monkeypatch.setattr(torch.cuda, "mem_get_info", lambda *a, **k: (100_000, 10 ** 12))
    need = 784 * 816 + 2 * 128 * RECORD_SIZE
    with pytest.raises(ValueError, match=rf"{need} bytes.*100000 bytes are free"):
        DeviceSLDataset.from_shards(shard_dir, chunk_records=128)


def test_append_raw_grows_and_keeps_the_order(positions):
    rec, packed = positions
    raw = to_device(rec)
    ds = DeviceSLDataset()
    assert len(ds) == 0 and ds.nbytes == 0
    parts = [np.arange(0, 600), np.arange(783, 100, -3), np.arange(1, 784, 2), np.zeros(0, np.int64), np.arange(600, 784)]
    for rows in parts:
        ds.append_raw(raw, rows)
    ds.check()
    order = np.concatenate(parts)
    assert len(ds) == len(order) > 1024                          # past the first allocation: the rows were moved
    assert np.array_equal(ds.packed.cpu().numpy().view(np.uint32), packed[order])
    with pytest.raises(IndexError, match="source row 784 out of range"):
        ds.append_raw(raw, [0, 784])
    bad = rec[:4].copy()
    bad["value"][2] = 7
    ds.append_raw(to_device(bad), [0, 1, 2, 3])
    with pytest.raises(ValueError, match=f"index {len(order) + 2}"):
        ds.check()


def test_prepare_sl_dataset_equals_the_shards_of_prepare_sl_data(tmp_path, monkeypatch):
    watched, shards = tmp_path / "cwd", tmp_path / "shards"
    watched.mkdir()
    monkeypatch.chdir(watched)
    files = [str(f) for f in FILES]
    kw = dict(min_ply=1, batch_envs=8, max_moves=MAX_MOVES, max_batch_positions=600)      # several batches
    ds, meta = prepare_sl_dataset(files, **kw)
    assert list(watched.iterdir()) == [], "prepare_sl_dataset wrote a file"
    want_meta = prep.prepare_sl_data(files, str(shards), shard_size=300, **kw)
    before = sorted((p.name, p.stat().st_size) for p in shards.iterdir())
    want = DeviceSLDataset.from_shards(shards, chunk_records=128)
    assert sorted((p.name, p.stat().st_size) for p in shards.iterdir()) == before and list(watched.iterdir()) == []
    assert len(ds) == len(want) == meta["num_positions"] == 784
    assert ds.packed.cpu().numpy().tobytes() == want.packed.cpu().numpy().tobytes()
    assert "num_shards" not in meta and set(meta) == set(want_meta) - {"num_shards"}
    for k in meta:
        assert meta[k] == want_meta[k], k


# ---------------------------------------------------------------------------------------------- the trainer
def run_epochs(shard_dir, sd0, amp, seed, orders=None):
    """Two epochs from the weights ``sd0``.  ``orders`` None: the shard path, its order fixed by seeding (the order is
    listed from the index loader under the same seed first); else the device-resident path over those orders."""
    model = build_model("se_resnet", MP)
    model.load_state_dict(sd0)
    model.to(DEV)
    cfg = SLConfig(data_dir=str(shard_dir), batch_size=256, total_epochs=5, use_amp=amp, device_resident=orders is not None)
    trainer = SLTrainer(model, cfg)
    assert (trainer.device_dataset is not None) == (orders is not None)
    used, metrics, states = [], [], []
    for ep in range(2):
        if orders is None:
            torch.manual_seed(seed + ep)
            used.append(torch.cat([b for b in trainer._index_loader]))
            torch.manual_seed(seed + ep)
        else:
            trainer._order_override = orders[ep]
            used.append(orders[ep])
        metrics.append(trainer.train_epoch())
        states.append({k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
    return used, metrics, states, trainer


@pytest.mark.parametrize("amp", [False, True], ids=["fp32", "bf16"])
def test_device_resident_epoch_equals_the_shard_epoch(shard_dir, amp):
    """Both paths hand identical tensors to identical launches in identical order; the bound is the shard path's own
    run-to-run distance (measured here: two runs from the same seed and weights), exact equality where that is zero."""
    torch.manual_seed(7)
    sd0 = {k: v.clone() for k, v in build_model("se_resnet", MP).state_dict().items()}
    orders, met_a, st_a, shard_trainer = run_epochs(shard_dir, sd0, amp, seed=31)
    orders_b, met_b, st_b, _ = run_epochs(shard_dir, sd0, amp, seed=31)
    assert all(torch.equal(a, b) for a, b in zip(orders, orders_b))
    assert all(sorted(o.tolist()) == list(range(784)) for o in orders) and not torch.equal(orders[0], orders[1])
    _, met_d, st_d, trainer = run_epochs(shard_dir, sd0, amp, seed=31, orders=orders)
    assert trainer._order_override is None
    for ep in range(2):
        assert met_d[ep].keys() == met_a[ep].keys() == {"policy_loss", "value_loss", "score_loss"}
        for k in met_a[ep]:
            own, dist = abs(met_a[ep][k] - met_b[ep][k]), abs(met_d[ep][k] - met_a[ep][k])
            print(f"amp={amp} epoch {ep} {k}: shard {met_a[ep][k]!r} device {met_d[ep][k]!r} own distance {own:.3e}")
            assert dist <= own, (ep, k, met_a[ep][k], met_d[ep][k], own)
        worst_own = worst = 0.0
        for k, v in st_a[ep].items():
            if v.dtype.is_floating_point:
                own = float((v - st_b[ep][k]).abs().max())
                dist = float((st_d[ep][k] - v).abs().max())
                worst_own, worst = max(worst_own, own), max(worst, dist)
                assert dist <= own, (ep, k, dist, own)
            else:
                assert torch.equal(st_d[ep][k], v), (ep, k)
        print(f"amp={amp} epoch {ep} parameters: shard path's own distance {worst_own:.3e}, device path {worst:.3e}")
    assert trainer.optimizer.param_groups[0]["lr"] == shard_trainer.optimizer.param_groups[0]["lr"]
    assert float(trainer.optimizer.state_dict()["state"][0]["step"]) == 8.0         # 4 batches (the last of 16) x 2 epochs
    assert trainer.scaler.get_scale() == shard_trainer.scaler.get_scale()


def test_device_epoch_draws_its_own_permutation_and_takes_a_dataset(shard_dir, monkeypatch):
    ds = DeviceSLDataset.from_shards(shard_dir)
    torch.manual_seed(5)
    model = build_model("se_resnet", MP).to(DEV)
    trainer = SLTrainer(model, SLConfig(data_dir="/nonexistent/never/read", batch_size=300), dataset=ds)
    assert trainer.device_dataset is ds and trainer.dataset is None
    seen = []
    real = DeviceSLDataset.gather
    monkeypatch.setattr(DeviceSLDataset, "gather", lambda self, idx, flag: seen.append(idx.cpu()) or real(self, idx, flag))
    torch.manual_seed(11)
    want = torch.randperm(784)
    torch.manual_seed(11)
    met = trainer.train_epoch()
    assert all(np.isfinite(v) for v in met.values())
    assert [len(s) for s in seen] == [300, 300, 184] and torch.equal(torch.cat(seen), want)
    trainer._order_override = torch.tensor([0, 784], dtype=torch.int64)           # the kernel's flag ends the epoch
    with pytest.raises(IndexError, match="outside the dataset"):
        trainer.train_epoch()


def test_device_resident_is_refused_off_the_fused_path_and_off_by_default(shard_dir, monkeypatch):
    with pytest.raises(ValueError, match="fused HIP path"):
        SLTrainer(build_model("se_resnet", MP), SLConfig(data_dir=str(shard_dir), device_resident=True))      # a CPU model
    with pytest.raises(ValueError, match="fused HIP path"):
        SLTrainer(build_model("se_resnet", MP), SLConfig(data_dir=str(shard_dir)),
                  dataset=DeviceSLDataset.from_shards(shard_dir))
    with monkeypatch.context() as m:                             # fp16 AMP has no fused path either
        m.setattr(torch.cuda, "is_bf16_supported", lambda *a, **k: False)
        with pytest.raises(ValueError, match="fused HIP path"):
            SLTrainer(build_model("se_resnet", MP).to(DEV), SLConfig(data_dir=str(shard_dir), use_amp=True, device_resident=True))
    assert SLConfig(data_dir="x").device_resident is False
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append(name) or real(name, *a))
    monkeypatch.setattr(DeviceSLDataset, "from_shards", lambda *a, **k: pytest.fail("the default config built a device dataset"))
    trainer = SLTrainer(build_model("se_resnet", MP).to(DEV), SLConfig(data_dir=str(shard_dir), batch_size=512))
    assert trainer.device_dataset is None and trainer._fused_path_available()
    trainer.train_epoch()
    assert "ka_policy_ce" in calls and "ka_sl_gather" not in calls and "ka_sl_pack" not in calls
