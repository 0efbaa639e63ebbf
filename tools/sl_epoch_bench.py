"""One SL epoch from shard files against one from the packed device-resident dataset (keisei_amd.sl.device_dataset), in the
same process: what ``SLTrainer.train_epoch()`` runs at when every minibatch comes through a memory map, a pinned copy and
an upload, and when it is one ``ka_sl_gather`` launch.

Data: the positions of tests/golden/g15_games.{sfen,csa} (prepared on the device), repeated to --positions and written
as shards of 8192 into a temporary directory -- about 1 GB at the default, the page cache warm after the write and the
warm-up epoch.  Workloads: se_resnet 6x128 at B = 2048 and 40x256 at B = 4096, bf16.  Per workload and path: one warm-up
epoch, then the best of --repeat epochs; the shard path and the device path alternate model by model in one job, so the
ratio is not a job-to-job comparison.  Two more legs run on the device-resident dataset: ``mirror``, the device epoch with
``SLConfig.mirror_augment`` (the gather reflects the drawn half of the positions), and ``evaluate``, ``SLTrainer.evaluate``
over the same positions (eval-mode forwards and ``ka_sl_eval``; --eval-batch rows per chunk, 0 = the training batch), timed
the same way.  --legs chooses among shard, device, mirror, evaluate.  Also reported: the ``DeviceSLDataset.from_shards`` load time (best of --repeat,
after a warm-up load) and the positions/s of the replay-and-pack step of ``prepare_sl_dataset`` on the synthetic games of
tools/sl_prepare_bench.py (as there, the games go in as action indices: parsing is not in the timing).
Clocks are not pinned.  One JSON line.

    python tools/sl_epoch_bench.py [--positions 65536] [--repeat 3] [--games 512] [--workloads 6x128,40x256]
                                   [--legs shard,device,mirror,evaluate] [--eval-batch 0]
"""
from __future__ import annotations

import argparse
import json
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from keisei_amd.sl import prepare as prep  # noqa: E402
from keisei_amd.sl.dataset import SLDataset  # noqa: E402
from keisei_amd.sl.device_dataset import DeviceSLDataset  # noqa: E402
from keisei_amd.sl.trainer import SLConfig, SLTrainer  # noqa: E402
from keisei_amd.training.model_registry import build_model  # noqa: E402

GOLDEN = ROOT / "tests" / "golden"
WORKLOADS = {   # name: (model parameters, batch size)
    "6x128": (dict(num_blocks=6, channels=128, se_reduction=16, global_pool_channels=128, policy_channels=32,
                   value_fc_size=256, score_fc_size=128, obs_channels=50), 2048),
    "40x256": (dict(num_blocks=40, channels=256, se_reduction=16, global_pool_channels=128, policy_channels=32,
                    value_fc_size=256, score_fc_size=128, obs_channels=50), 4096),
}
SHARD = 8192


def write_shards(out: Path, positions: int) -> int:
    """The fixture's positions, repeated, as shard files; returns how many distinct positions there are."""
    with tempfile.TemporaryDirectory() as first:
        prep.prepare_sl_data([str(GOLDEN / "g15_games.sfen"), str(GOLDEN / "g15_games.csa")], first, min_ply=1)
        base = SLDataset(Path(first))
        rec = np.concatenate([np.asarray(base._records(k)) for k in range(len(base.shards))])
    reps = np.resize(np.arange(len(rec)), positions)
    for k, at in enumerate(range(0, positions, SHARD)):
        rec[reps[at:at + SHARD]].tofile(out / f"shard_{k:03d}.bin")
    return len(rec)


def best_epoch(trainer: SLTrainer, repeat: int):
    trainer.train_epoch()                                       # warm-up: page cache, allocator, kernel loading
    best, metrics = float("inf"), None
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        metrics = trainer.train_epoch()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best, metrics


def timed(fn, repeat: int) -> float:
    fn()
    best = float("inf")
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return best


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--positions", type=int, default=65536)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--games", type=int, default=512, help="synthetic games of the prepare_sl_dataset timing; 0 skips it")
    ap.add_argument("--moves", type=int, default=120)
    ap.add_argument("--workloads", default="6x128,40x256")
    ap.add_argument("--legs", default="shard,device,mirror,evaluate")
    ap.add_argument("--eval-batch", type=int, default=0, help="rows per evaluate() chunk; 0 = the workload's training batch")
    args = ap.parse_args()
    legs = args.legs.split(",")
    unknown = set(legs) - {"shard", "device", "mirror", "evaluate"}
    if unknown:
        ap.error(f"unknown legs {sorted(unknown)}")
    out = {"metric": "sl_epoch_positions_per_s", "positions": args.positions, "repeat": args.repeat, "dtype": "bf16"}
    with tempfile.TemporaryDirectory() as tmp:
        out["distinct_positions"] = write_shards(Path(tmp), args.positions)
        out["shard_bytes"] = sum(p.stat().st_size for p in Path(tmp).glob("shard_*.bin"))
        held = {}
        out["from_shards_s"] = round(timed(lambda: held.update(ds=DeviceSLDataset.from_shards(tmp)), args.repeat), 4)
        dataset = held["ds"]
        out["packed_bytes"] = dataset.nbytes
        out["from_shards_positions_per_s"] = round(args.positions / out["from_shards_s"])
        for name in args.workloads.split(","):
            params, batch = WORKLOADS[name]
            row = {"batch": batch}
            for path in legs:
                torch.manual_seed(0)
                model = build_model("se_resnet", params).to("cuda")
                cfg = SLConfig(data_dir=tmp, batch_size=batch, use_amp=True, mirror_augment=path == "mirror")
                trainer = SLTrainer(model, cfg, dataset=None if path == "shard" else dataset)
                assert trainer._fused_path_available() and (trainer.device_dataset is not None) == (path != "shard")
                if path == "evaluate":
                    held = {}
                    chunk = args.eval_batch or batch
                    seconds = timed(lambda: held.update(m=trainer.evaluate(dataset, batch_size=chunk)), args.repeat)
                    metrics = held["m"]
                    row["evaluate_batch"] = chunk
                    row["evaluate_policy_top1"] = round(metrics["policy_top1"], 4)
                else:
                    seconds, metrics = best_epoch(trainer, args.repeat)
                row[f"{path}_s"] = round(seconds, 4)
                row[f"{path}_positions_per_s"] = round(args.positions / seconds)
                row[f"{path}_policy_loss"] = round(metrics["policy_loss"], 4)
                del trainer, model
                torch.cuda.empty_cache()
            for a, b in (("device", "shard"), ("mirror", "device"), ("evaluate", "device")):
                if f"{a}_s" in row and f"{b}_s" in row:
                    row[f"{a}_over_{b}"] = round(row[f"{b}_s"] / row[f"{a}_s"], 3)
            out[name] = row
        del dataset, held
    if args.games:
        from sl_prepare_bench import synthetic_games

        games = synthetic_games(args.games, args.moves)
        batch = prep.ReplayBatch.build(games)
        replay = prep._DeviceReplay(args.games, max(len(g[0]) for g in games))
        state = {"raw": None}

        def replay_and_pack():
            ds = DeviceSLDataset(replay.device)
            state["raw"], _, _ = prep._replay_onto(ds, replay, batch, state["raw"])
            ds.check()
            state["n"] = len(ds)

        seconds = timed(replay_and_pack, args.repeat)
        out["prepare_sl_dataset"] = {"games": args.games, "positions": state["n"], "seconds": round(seconds, 4),
                                     "positions_per_s": round(state["n"] / seconds)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
