"""GPU: the reflecting gather ``ka_sl_gather_aug`` (csrc/sl_data.hip) against its numpy restatement
``mirror_records(unpack_records(...))`` / ``sl_mirror_draw`` byte for byte, and the device epoch of ``SLTrainer`` with
``mirror_augment`` against a device epoch over host-reflected records.  Everything up to the trainer is a copy of bits and
the trainer runs identical launches on identical tensors: equality is exact."""
import numpy as np
import pytest
import torch

from keisei_amd import _lib
from keisei_amd.sl import DeviceSLDataset
from keisei_amd.sl import prepare as prep
from keisei_amd.sl.dataset import OBS_SIZE, RECORD_SIZE, _RECORD
from keisei_amd.sl.device_dataset import mirror_records, pack_records, sl_mirror_draw, unpack_records
from keisei_amd.sl.trainer import SLConfig, SLTrainer
from keisei_amd.training.model_registry import build_model
from oracle import shogi as so
from sl_prepare_helpers import fixture_games

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 0xA5
SEEDS = (0, 20260, -3, 2 ** 64 - 1)                  # tests/test_sl_mirror_cpu.py: both outcomes occur under each
MP = dict(num_blocks=2, channels=32, se_reduction=8, global_pool_channels=16, policy_channels=8,
          value_fc_size=32, score_fc_size=16, obs_channels=50)


@pytest.fixture(scope="module")
def positions(golden):
    """The 784 fixture positions, their packed rows and their host-reflected records."""
    games, _ = fixture_games(golden("g15_sl_prepare"), 512)
    batch = prep.ReplayBatch.build(games)
    buf, valid_len, _, _ = prep._replay_host(batch, so.OracleVecEnv(batch.num_envs, 512))
    rec = buf[prep._kept_rows(batch, valid_len)].copy()
    assert len(rec) == 784
    packed, first_bad = pack_records(rec)
    assert first_bad is None
    mirrored = mirror_records(unpack_records(packed))
    for a in (rec, packed, mirrored):
        a.setflags(write=False)
    return rec, packed, mirrored


def guarded(nbytes: int, pad: int = 16):
    whole = torch.full((nbytes + 2 * pad,), GUARD, dtype=torch.uint8, device=DEV)
    return whole, whole[pad:pad + nbytes]


def guards_intact(whole: torch.Tensor, nbytes: int, pad: int = 16) -> bool:
    host = whole.cpu().numpy()
    return bool((host[:pad] == GUARD).all() and (host[pad + nbytes:] == GUARD).all())


def run_gather(packed, n, idx, mode=None, seed=0, epoch=0):
    """``ka_sl_gather_aug`` (``ka_sl_gather`` for mode None) into guarded outputs: ``(records, flag)``."""
    B = len(idx)
    pk = torch.from_numpy(np.array(packed).view(np.int32)).to(DEV)
    sizes = (B * OBS_SIZE * 4, B * 8, B * 8, B * 4)
    bufs = [guarded(s) for s in sizes]
    obs = bufs[0][1].view(torch.float32).view(B, 50, 9, 9)
    policy, value = bufs[1][1].view(torch.int64), bufs[2][1].view(torch.int64)
    score = bufs[3][1].view(torch.float32)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    index = torch.tensor(idx, dtype=torch.int64, device=DEV)
    if mode is None:
        _lib.call("ka_sl_gather", pk, n, index, B, obs, policy, value, score, flag, _lib.stream_ptr())
    else:
        seed64 = seed & (2 ** 64 - 1)
        _lib.call("ka_sl_gather_aug", pk, n, index, B, obs, policy, value, score, flag, mode,
                  seed64 - 2 ** 64 if seed64 >> 63 else seed64, epoch, _lib.stream_ptr())
    for (whole, _), s in zip(bufs, sizes):
        assert guards_intact(whole, s), "the gather wrote outside an output"
    got = np.zeros(B, dtype=_RECORD)
    got["obs"] = obs.cpu().numpy().reshape(B, OBS_SIZE)
    got["policy"], got["value"], got["score"] = policy.cpu().numpy(), value.cpu().numpy(), score.cpu().numpy()
    return got, int(flag.item())


def expected(rec, mirrored, idx, reflect):
    want = rec[idx].copy()
    want[reflect] = mirrored[idx][reflect]
    return want


def batch_indices(B, n):
    rng = np.random.default_rng(B)
    idx = rng.integers(0, n, B)
    if B >= 3:
        idx[0], idx[1], idx[B - 1] = 0, n - 1, n - 1             # the ends, one of them repeated
    if B >= 63:
        idx[10:40] = rng.integers(0, 8, 30)                      # 30 draws from 8 rows: repeats
    return idx


# ---------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("B", [1, 63, 64, 65, 257])
def test_gather_aug_equals_the_host_reflection(positions, B, mode):
    rec, packed, mirrored = positions
    n = len(rec)
    seed, epoch = SEEDS[B % 4], B % 3
    idx = batch_indices(B, n)
    batches = [idx]
    if mode == 2 and B == 1:                                     # one row cannot hold both outcomes: two batches of one
        drawn = sl_mirror_draw(seed, epoch, np.arange(n))
        batches = [np.array([np.nonzero(drawn)[0][0]]), np.array([np.nonzero(~drawn)[0][0]])]
    seen = set()
    for idx in batches:
        reflect = {0: np.zeros(len(idx), bool), 1: np.ones(len(idx), bool), 2: sl_mirror_draw(seed, epoch, idx)}[mode]
        seen |= set(reflect.tolist())
        got, flag = run_gather(packed, n, idx.tolist(), mode, seed, epoch)
        assert flag == 0
        assert got.tobytes() == expected(rec, mirrored, idx, reflect).tobytes()
        if mode == 0:
            plain, flag = run_gather(packed, n, idx.tolist())
            assert flag == 0 and got.tobytes() == plain.tobytes() == rec[idx].tobytes()
    assert seen == {0: {False}, 1: {True}, 2: {False, True}}[mode]


def test_the_draw_depends_on_seed_epoch_and_position_only(positions):
    rec, packed, mirrored = positions
    n = len(rec)
    idx = np.arange(0, n, 3)
    base, _ = run_gather(packed, n, idx.tolist(), 2, 20260, 1)
    # the same positions in another order and another batch geometry: every position is treated as before
    order = np.random.default_rng(1).permutation(len(idx))
    again, _ = run_gather(packed, n, idx[order][:100].tolist(), 2, 20260, 1)
    assert again.tobytes() == base[order][:100].tobytes()
    for seed, epoch in ((20260, 2), (20261, 1)):
        other, _ = run_gather(packed, n, idx.tolist(), 2, seed, epoch)
        assert other.tobytes() == expected(rec, mirrored, idx, sl_mirror_draw(seed, epoch, idx)).tobytes() != base.tobytes()


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_gather_aug_flags_an_index_outside_the_dataset(positions, mode):
    rec, packed, mirrored = positions
    n = len(rec)
    idx = np.array([3, n, 0, n - 1, -1, 3, 17])
    inside = np.array([3, 0, 0, n - 1, 0, 3, 17])
    got, flag = run_gather(packed, n, idx.tolist(), mode, -3, 2)
    assert flag == 2
    reflect = {0: np.zeros(7, bool), 1: np.ones(7, bool), 2: sl_mirror_draw(-3, 2, inside)}[mode]
    want = expected(rec, mirrored, inside, reflect)
    want[[1, 4]] = np.zeros(2, dtype=_RECORD)                    # zero observation, targets of 0, never reflected
    assert got.tobytes() == want.tobytes()
    got, flag = run_gather(packed, 10, [9, 10], mode, -3, 2)      # a dataset shorter than its allocation
    assert flag == 1 and got[1:].tobytes() == bytes(RECORD_SIZE)
    nine = {0: False, 1: True, 2: bool(sl_mirror_draw(-3, 2, 9))}[mode]
    assert got[:1].tobytes() == (mirrored if nine else rec)[9:10].tobytes()


def test_gather_aug_refuses_a_bad_mode_or_epoch(positions):
    rec, packed, _ = positions
    for mode, epoch, text in ((3, 0, "mode 3"), (-1, 0, "mode -1"), (2, -1, "epoch -1")):
        with pytest.raises(_lib.KeiseiHipError, match=text):
            run_gather(packed, len(rec), [0], mode, 0, epoch)


def to_device(records) -> torch.Tensor:
    return torch.from_numpy(np.frombuffer(records.tobytes(), dtype=np.uint8).copy()).to(DEV)


def dataset_of(records) -> DeviceSLDataset:
    ds = DeviceSLDataset()
    ds.append_raw(to_device(records), np.arange(len(records)))
    ds.check()
    return ds


def test_dataset_gather_takes_the_mirror_arguments(positions):
    rec, packed, mirrored = positions
    ds = dataset_of(rec)
    idx = np.arange(5, 300, 7)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    index = torch.from_numpy(idx).to(DEV)
    for kw, reflect in (({}, np.zeros(len(idx), bool)), (dict(mirror=1), np.ones(len(idx), bool)),
                        (dict(mirror=2, seed=2 ** 64 - 1, epoch=4), sl_mirror_draw(2 ** 64 - 1, 4, idx)),
                        (dict(mirror=2, seed=-3, epoch=1), sl_mirror_draw(-3, 1, idx))):
        got = ds.gather(index, flag, **kw)
        want = expected(rec, mirrored, idx, reflect)
        assert got["observation"].cpu().numpy().tobytes() == want["obs"].tobytes(), kw
        assert got["policy_target"].cpu().numpy().tolist() == want["policy"].tolist(), kw
        assert got["value_target"].cpu().numpy().tolist() == want["value"].tolist(), kw
        assert got["score_target"].cpu().numpy().tobytes() == want["score"].tobytes(), kw
    assert int(flag.item()) == 0
    for kw in (dict(mirror=3), dict(mirror=2, epoch=-1), dict(mirror=2, epoch=2 ** 31)):
        with pytest.raises(ValueError):
            ds.gather(index, flag, **kw)


# ---------------------------------------------------------------------------------------------- the trainer
def run_epochs(sd0, datasets, orders, **config):
    """Two device epochs from the weights ``sd0``: epoch e over ``datasets[e]`` in the order ``orders[e]``."""
    model = build_model("se_resnet", MP)
    model.load_state_dict(sd0)
    model.to(DEV)
    trainer = SLTrainer(model, SLConfig(data_dir="/nonexistent/never/read", batch_size=256, total_epochs=5, **config),
                        dataset=datasets[0])
    metrics, states = [], []
    for ep in range(2):
        trainer.device_dataset = datasets[ep]
        trainer._order_override = orders[ep]
        metrics.append(trainer.train_epoch())
        states.append({k: v.detach().cpu().clone() for k, v in model.state_dict().items()})
    return metrics, states, trainer


def test_mirror_augmented_epoch_equals_an_epoch_over_host_reflected_records(positions, monkeypatch):
    rec, _, mirrored = positions
    n, seed = len(rec), 20260
    torch.manual_seed(7)
    sd0 = {k: v.clone() for k, v in build_model("se_resnet", MP).state_dict().items()}
    orders = [torch.from_numpy(np.random.default_rng(40 + ep).permutation(n)) for ep in range(2)]
    draws = [sl_mirror_draw(seed, ep, np.arange(n)) for ep in range(2)]
    assert all(d.any() and not d.all() for d in draws)
    assert not np.array_equal(draws[0], draws[1])                 # a second epoch draws differently from the first
    plain = dataset_of(rec)
    calls = []
    real = DeviceSLDataset.gather
    monkeypatch.setattr(DeviceSLDataset, "gather", lambda self, idx, flag, **kw: calls.append(kw) or real(self, idx, flag, **kw))
    met_a, st_a, trainer = run_epochs(sd0, [plain, plain], orders, mirror_augment=True, mirror_seed=seed)
    assert trainer.epochs_done == 2 and trainer._order_override is None
    assert calls == [dict(mirror=2, seed=seed, epoch=0)] * 4 + [dict(mirror=2, seed=seed, epoch=1)] * 4
    del calls[:]
    # the comparison run: no augmentation, each epoch over the records reflected on the host as that epoch's draw says
    reflected = [dataset_of(expected(rec, mirrored, np.arange(n), draws[ep])) for ep in range(2)]
    met_b, st_b, _ = run_epochs(sd0, reflected, orders)
    assert calls == [{}] * 8
    met_c, st_c, _ = run_epochs(sd0, [plain, plain], orders)      # and without any reflection the weights differ
    for ep in range(2):
        assert met_a[ep] == met_b[ep], (ep, met_a[ep], met_b[ep])
        for k, v in st_a[ep].items():
            assert torch.equal(v, st_b[ep][k]), (ep, k)
        assert any(not torch.equal(v, st_c[ep][k]) for k, v in st_a[ep].items())
