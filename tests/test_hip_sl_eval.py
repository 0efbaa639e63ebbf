"""GPU: the held-out evaluation kernel ``ka_sl_eval`` (csrc/loss.hip) against numpy -- hit counts exactly, by the
stable-sort rule; loss sums against float64 within the bar the loss kernels meet, 1e-5 relative -- then
``SLTrainer.evaluate`` against numpy over the logits of the model's own eval forward, and ``DeviceSLDataset.view``."""
import numpy as np
import pytest
import torch

from keisei_amd import _lib
from keisei_amd.sl import DeviceSLDataset
from keisei_amd.sl import prepare as prep
from keisei_amd.sl.device_dataset import mirror_records
from keisei_amd.sl.trainer import SLConfig, SLTrainer
from keisei_amd.training.model_registry import build_model
from oracle import shogi as so
from sl_prepare_helpers import fixture_games

pytestmark = pytest.mark.gpu
DEV = "cuda"
RTOL = 1e-5                                          # "losses 1e-5"
CASES = 6
MP = dict(num_blocks=2, channels=32, se_reduction=8, global_pool_channels=16, policy_channels=8,
          value_fc_size=32, score_fc_size=16, obs_channels=50)


# ---------------------------------------------------------------------------------------------- numpy
def ranks_of(logits, targets):
    """The target's place in a stable descending sort: #{j : z_j > z_t} + #{j < t : z_j == z_t}, on the fp32 values."""
    zt = logits[np.arange(len(targets)), targets][:, None]
    before = np.arange(logits.shape[1])[None, :] < targets[:, None]
    return (logits > zt).sum(axis=1) + ((logits == zt) & before).sum(axis=1)


def reference(logits, vlogits, score, tp, tv, ts, k):
    """``(int counts [positions, top1, topk, value_correct], float64 sums [policy CE, value CE, squared score error])``."""
    z, v = logits.astype(np.float64), vlogits.astype(np.float64)
    rows = np.arange(len(tp))

    def lse(x):
        m = x.max(axis=1, keepdims=True)
        return m[:, 0] + np.log(np.exp(x - m).sum(axis=1))

    rank = ranks_of(logits, tp)
    pred = np.where((vlogits[:, 0] >= vlogits[:, 1]) & (vlogits[:, 0] >= vlogits[:, 2]), 0,
                    np.where(vlogits[:, 1] >= vlogits[:, 2], 1, 2))
    counts = [len(tp), int((rank == 0).sum()), int((rank < k).sum()), int((pred == tv).sum())]
    d = score.astype(np.float32) - ts.astype(np.float32)         # the difference is formed in fp32, as ka_value_loss forms it
    sums = [float((lse(z) - z[rows, tp]).sum()), float((lse(v) - v[rows, tv]).sum()), float((d.astype(np.float64) ** 2).sum())]
    return counts, sums


def crafted(B, A, k, rng, shift=0):
    """Random logits with row r shaped by case (r + shift) % 6: ties above and below the target's index; the target at 0; the
    target at A - 1 behind an earlier tie; rank exactly k - 1; rank exactly k; -inf entries.  Ranks come from ``ranks_of``."""
    logits = rng.standard_normal((B, A)).astype(np.float32)
    tp = rng.integers(0, A, B)
    for r in range(B):
        case = (r + shift) % CASES
        top = np.float32(logits[r].max() + 1.0)
        if case == 0:
            t = tp[r] = rng.integers(1, A - 1)
            logits[r, [t - 1, t, t + 1]] = top                   # equal logits at a lower and at a higher index: rank 1
            if t >= 2:
                logits[r, 0] = top                               # and another one below: rank 2
        elif case == 1:
            tp[r] = 0
            logits[r, [0, A - 1]] = top                          # the tie lies above the target's index: rank 0
        elif case == 2:
            tp[r] = A - 1
            logits[r, [A // 2, A - 1]] = top                     # the tie lies below it: rank 1
        elif case in (3, 4):
            order = rng.permutation(A)                           # distinct values: order[j] of them are greater than z_j
            logits[r] = (A - order).astype(np.float32) / np.float32(A)
            want = min(k - 1 if case == 3 else k, A - 1)
            tp[r] = int(np.nonzero(order == want)[0][0])
        else:
            off = rng.choice(np.delete(np.arange(A), tp[r]), size=max(1, A // 3), replace=False)
            logits[r, off] = -np.inf
    vlogits = rng.standard_normal((B, 3)).astype(np.float32)
    vlogits[::4, 1] = vlogits[::4, 0]                            # value ties: the argmax rule takes the lower class
    vlogits[::7, 2] = vlogits[::7, 1]
    score = rng.standard_normal(B).astype(np.float32)
    return logits, vlogits, score, tp.astype(np.int64), rng.integers(0, 3, B).astype(np.int64), rng.standard_normal(B).astype(np.float32)


# ---------------------------------------------------------------------------------------------- the kernel
def run_eval(batches, k, acc=None, flags=None):
    """Adds every batch (logits, vlogits, score, tp, tv, ts) into one accumulator: ``(acc int64[8] on the host, flags)``."""
    acc = torch.zeros(8, dtype=torch.int64, device=DEV) if acc is None else acc
    flags = torch.zeros(2, dtype=torch.int32, device=DEV) if flags is None else flags
    for logits, vlogits, score, tp, tv, ts in batches:
        B, A = logits.shape
        dev = [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) for x in (logits, vlogits, score, tp, tv, ts)]
        rowloss = torch.full((B + 2,), 777.0, device=DEV)        # one guard word on either side of the workspaces
        rank = torch.full((B + 2,), -777, dtype=torch.int32, device=DEV)
        _lib.call("ka_sl_eval", *dev, B, A, k, rowloss[1:B + 1], rank[1:B + 1], acc, flags, _lib.stream_ptr())
        assert rowloss[[0, B + 1]].tolist() == [777.0, 777.0] and rank[[0, B + 1]].tolist() == [-777, -777]
    return acc.cpu().numpy(), flags.cpu().tolist()


def split(acc):
    return acc[:4].tolist(), acc[4:].view(np.float64).tolist()


def close(got, want):
    return abs(got - want) <= RTOL * abs(want)


@pytest.mark.parametrize("B", [1, 3, 1025])
@pytest.mark.parametrize("A", [5, 300, 11259])
def test_sl_eval_counts_exactly_and_sums_within_the_loss_bar(A, B):
    k = 3 if A == 5 else 5
    rng = np.random.default_rng(A * 10000 + B)
    batches = [crafted(B, A, k, rng, shift) for shift in range(CASES if B < CASES else 1)]       # every case at every shape
    ranks = np.concatenate([ranks_of(b[0], b[3]) for b in batches])
    assert {0, 1, k - 1, k} <= set(ranks.tolist()) and (ranks >= k).any()
    whole = [np.concatenate([b[i] for b in batches]) for i in range(6)]
    counts, sums = reference(*whole, k)
    acc, flags = run_eval(batches, k)
    got_counts, got_sums = split(acc)
    print(f"A={A} B={B}: counts {got_counts} want {counts}; sums {got_sums[:3]} want {sums}; "
          f"relative {[abs(g - w) / abs(w) for g, w in zip(got_sums, sums)]}")
    assert flags == [0, 0]
    assert got_counts == counts
    assert all(close(g, w) for g, w in zip(got_sums, sums)) and got_sums[3] == 0.0
    again, _ = run_eval(batches, k)
    assert again.tobytes() == acc.tobytes()                      # two runs: the same bits


def test_sl_eval_accumulates_batches_of_different_sizes():
    rng = np.random.default_rng(5)
    A, k = 300, 5
    first, second = crafted(1025, A, k, rng), crafted(3, A, k, rng, shift=2)
    counts, sums = reference(*[np.concatenate([first[i], second[i]]) for i in range(6)], k)
    acc, flags = run_eval([first, second], k)
    got_counts, got_sums = split(acc)
    assert flags == [0, 0] and got_counts == counts and got_counts[0] == 1028
    assert all(close(g, w) for g, w in zip(got_sums, sums))
    # k = 1 makes top-k top-1, k = A counts every position
    top1 = int((ranks_of(first[0], first[3]) == 0).sum())
    assert split(run_eval([first], 1)[0])[0][1:3] == [top1, top1]
    assert split(run_eval([first], A)[0])[0][2] == 1025
    for bad in (0, A + 1):
        with pytest.raises(_lib.KeiseiHipError, match="k "):
            run_eval([second], bad)


def test_sl_eval_flags_nan_and_targets_outside_their_range():
    rng = np.random.default_rng(9)
    A, k, B = 300, 5, 65
    clean = crafted(B, A, k, rng)
    for where in ("logits", "value", "score"):
        logits, vlogits, score, tp, tv, ts = (x.copy() for x in clean)
        if where == "logits":
            logits[40, 17] = np.nan
        elif where == "value":
            vlogits[40, 1] = np.nan
        else:
            score[40] = np.nan
        acc, flags = run_eval([(logits, vlogits, score, tp, tv, ts)], k)
        assert flags == [1, 0], where
        assert np.isnan(split(acc)[1][{"logits": 0, "value": 1, "score": 2}[where]])
    keep = np.ones(B, bool)
    keep[[3, 50]] = False
    for bad in (A, -1, 2 ** 40):                                 # a policy target outside [0, A): no policy term for that row
        logits, vlogits, score, tp, tv, ts = (x.copy() for x in clean)
        tp[[3, 50]] = bad
        acc, flags = run_eval([(logits, vlogits, score, tp, tv, ts)], k)
        counts, sums = reference(*clean, k)
        kept, kept_sums = reference(*[x[keep] for x in clean], k)
        got_counts, got_sums = split(acc)
        assert flags == [0, 1], bad
        assert got_counts == [B, kept[1], kept[2], counts[3]]
        assert close(got_sums[0], kept_sums[0]) and close(got_sums[1], sums[1]) and close(got_sums[2], sums[2])
    for bad in (3, -1):                                          # a value target outside {0, 1, 2}: no value term
        logits, vlogits, score, tp, tv, ts = (x.copy() for x in clean)
        tv[[3, 50]] = bad
        acc, flags = run_eval([(logits, vlogits, score, tp, tv, ts)], k)
        counts, sums = reference(*clean, k)
        kept, kept_sums = reference(*[x[keep] for x in clean], k)
        got_counts, got_sums = split(acc)
        assert flags == [0, 1], bad
        assert got_counts == [B, counts[1], counts[2], kept[3]]
        assert close(got_sums[0], sums[0]) and close(got_sums[1], kept_sums[1]) and close(got_sums[2], sums[2])


# ---------------------------------------------------------------------------------------------- the dataset view
@pytest.fixture(scope="module")
def records(golden):
    games, _ = fixture_games(golden("g15_sl_prepare"), 512)
    batch = prep.ReplayBatch.build(games)
    buf, valid_len, _, _ = prep._replay_host(batch, so.OracleVecEnv(batch.num_envs, 512))
    rec = buf[prep._kept_rows(batch, valid_len)].copy()
    assert len(rec) == 784
    rec.setflags(write=False)
    return rec


def to_device(rec) -> torch.Tensor:
    return torch.from_numpy(np.frombuffer(rec.tobytes(), dtype=np.uint8).copy()).to(DEV)


def dataset_of(rec) -> DeviceSLDataset:
    ds = DeviceSLDataset()
    ds.append_raw(to_device(rec), np.arange(len(rec)))
    ds.check()
    return ds


def test_view_shares_memory_and_is_read_only(records):
    ds = dataset_of(records)
    tail = ds.view(600, 784)
    assert len(tail) == 184 and tail.nbytes == 184 * 816 and tail.device == ds.device
    assert tail.packed.data_ptr() == ds.packed[600].data_ptr() and tail.packed.shape == (184, 204)
    assert torch.equal(tail.packed, ds.packed[600:784])
    got, want = tail.read_batch([0, 183, 5]), ds.read_batch([600, 783, 605])
    assert all(torch.equal(got[key], want[key]) for key in want)
    with pytest.raises(IndexError, match="index 184 out of range for dataset with 184 positions"):
        tail.read_batch([184])
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    row = tail.gather(torch.tensor([184, 0], device=DEV), flag)  # the parent's row 784 would lie past the view's end
    assert int(flag.item()) == 1 and not row["observation"][0].any() and row["observation"][1].any()
    ds.packed[700, 200] += 1                                     # no copy: a write to the parent shows in the view
    assert int(tail.packed[100, 200]) == int(ds.packed[700, 200])
    ds.packed[700, 200] -= 1
    inner = tail.view(10, 20)
    assert inner.packed.data_ptr() == ds.packed[610].data_ptr() and len(inner) == 10
    assert len(ds.view(0, 0)) == 0 and len(ds.view(784, 784)) == 0 and len(ds.view(0, 784)) == 784
    for v in (tail, inner):
        with pytest.raises(ValueError, match="view"):
            v.append_raw(to_device(records[:2]), [0, 1])
    assert len(tail) == 184 and len(ds) == 784
    for lo, hi in ((-1, 5), (0, 785), (10, 9), (785, 785)):
        with pytest.raises(IndexError, match="out of range"):
            ds.view(lo, hi)
    ds.append_raw(to_device(records[:2]), [0, 1])                # the parent still grows
    assert len(ds) == 786


# ---------------------------------------------------------------------------------------------- the trainer
def snapshot(trainer):
    opt = trainer.optimizer.state_dict()
    tensors = {f"model.{k}": v.detach().clone() for k, v in trainer.model.state_dict().items()}
    for i, st in opt["state"].items():
        tensors.update({f"opt.{i}.{k}": v.detach().clone() for k, v in st.items() if torch.is_tensor(v)})
    plain = (opt["param_groups"], trainer.scheduler.state_dict(), trainer.scaler.state_dict(), trainer.epochs_done,
             [m.training for m in trainer.model.modules()])
    return tensors, repr(plain)


def same(a, b):
    return a[1] == b[1] and a[0].keys() == b[0].keys() and all(torch.equal(v, b[0][k]) for k, v in a[0].items())


def test_evaluate_against_numpy_over_the_models_own_eval_forward(records):
    ds = dataset_of(records)
    train, held = ds.view(0, 600), ds.view(600, 784)
    torch.manual_seed(3)
    model = build_model("se_resnet", MP).to(DEV)
    trainer = SLTrainer(model, SLConfig(data_dir="/nonexistent/never/read", batch_size=256, total_epochs=5), dataset=train,
                        eval_dataset=held)
    trainer.train_epoch()                                        # optimiser state and BatchNorm statistics to preserve
    assert model.training
    before = snapshot(trainer)
    names = []
    real = _lib.call
    _lib.call = lambda name, *a: names.append(name) or real(name, *a)
    try:
        got = trainer.evaluate(batch_size=80, topk=5)            # 184 = 80 + 80 + 24
    finally:
        _lib.call = real
    assert same(snapshot(trainer), before), "evaluate() changed the training state"
    assert names.count("ka_sl_gather") == 3 and names.count("ka_sl_eval") == 3
    assert not {"ka_policy_ce", "ka_value_loss", "ka_clip_adam_step", "ka_sl_gather_aug"} & set(names)
    assert set(got) == {"policy_loss", "value_loss", "score_loss", "policy_top1", "policy_topk", "value_accuracy", "positions"}

    # the same chunks through the model's eval forward, read back
    model.eval()
    outs = []
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    with torch.no_grad():
        for lo in range(0, 184, 80):
            b = held.gather(torch.arange(lo, min(lo + 80, 184), device=DEV), flag)
            out = model(b["observation"])
            outs.append([x.float().cpu().numpy() for x in (out.policy_logits.reshape(len(b["policy_target"]), -1),
                                                            out.value_logits, out.score_lead.reshape(-1))])
    model.train()
    logits, vlogits, score = (np.concatenate([o[i] for o in outs]) for i in range(3))
    tail = records[600:]
    counts, sums = reference(logits, vlogits, score, tail["policy"], tail["value"], tail["score"], 5)
    print(f"evaluate: {got}; numpy counts {counts} sums {sums}")
    assert got["positions"] == 184 == counts[0]
    assert [got["policy_top1"], got["policy_topk"], got["value_accuracy"]] == [c / 184 for c in counts[1:]]
    for key, want in zip(("policy_loss", "value_loss", "score_loss"), sums):
        assert close(got[key], want / 184), key

    # a k at which a freshly initialised model does hit: the count is still the stable-sort rule's
    wide = trainer.evaluate(batch_size=80, topk=3000)
    hits = int((ranks_of(logits, tail["policy"].astype(np.int64)) < 3000).sum())
    assert 0 < hits < 184 and wide["policy_topk"] == hits / 184 and wide["policy_loss"] == got["policy_loss"]

    # an explicit dataset, the default chunk, eval mode kept; top-1 of k = 1
    model.eval()
    again = trainer.evaluate(held, topk=1)
    assert not model.training and not any(m.training for m in model.modules())
    model.train()
    assert again["policy_topk"] == again["policy_top1"] == got["policy_top1"] and again["positions"] == 184
    assert close(again["policy_loss"], got["policy_loss"])       # one chunk of 184 against three: sums over positions

    # the reflected set is the set of host-reflected records
    mirrored = trainer.evaluate(batch_size=80, mirror=True)
    assert mirrored == trainer.evaluate(dataset_of(mirror_records(tail)), batch_size=80)
    assert mirrored != got
    assert same(snapshot(trainer), before)

    with pytest.raises(ValueError, match="topk"):
        trainer.evaluate(topk=0)
    with pytest.raises(ValueError, match="topk"):
        trainer.evaluate(topk=11260)
    with pytest.raises(ValueError, match="batch_size"):
        trainer.evaluate(batch_size=0)
    assert same(snapshot(trainer), before) and model.training
    assert trainer.evaluate(ds.view(0, 0))["positions"] == 0

    # a NaN among the logits sets the kernel's flag, and the flag ends the evaluation
    bias = model.policy_conv2.bias
    kept = bias.detach().clone()
    with torch.no_grad():
        bias[7] = float("nan")
    model._hip_engine.notify_weights_updated()
    with pytest.raises(ValueError, match="non-finite"):
        trainer.evaluate(batch_size=80)
    with torch.no_grad():
        bias.copy_(kept)
    model._hip_engine.notify_weights_updated()
    assert same(snapshot(trainer), before) and model.training
    assert trainer.evaluate(batch_size=80, topk=5) == got
    with pytest.raises(ValueError, match="needs a dataset"):
        SLTrainer(model, SLConfig(data_dir="/nonexistent/never/read"), dataset=train).evaluate()
