"""SL shard preparation on the device (keisei_amd.sl.prepare: ka_sl_replay_plan + ka_shogi_env_step + ka_sl_replay_record
per ply, no host read inside a batch) against the same replay done with what the package had before it: VecEnv(
output="numpy").step ply by ply from Python, the records assembled in numpy (``_replay_host`` over that env), write_shard.

The games are synthetic: --games seeded random legal playouts of the CPU env oracle, lengths uniform in
[--moves * 3/4, --moves * 5/4] (shorter where the rules end the playout).  They go in as action indices: parsing and the
USI conversion are not in the timing.  One batch holds them all (``batch_envs`` = --games).

Reported, after one warm-up run each (kernel loading, buffer growth), over --repeat runs: positions/s of the batch
without file writes (replay, the read of the state, the copy to pinned host memory, dropping the rows of cut moves) and
with them (the shard writer on top, into a temporary directory), for both paths; the ratio; the share of filler steps.
Clocks are not pinned.  One JSON line.

    python tools/sl_prepare_bench.py [--games 512] [--moves 120] [--repeat 3] [--shard-size 100000]
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

import numpy as np  # noqa: E402
import torch  # noqa: E402

from keisei_amd.shogi_gym import VecEnv  # noqa: E402
from keisei_amd.sl import prepare as prep  # noqa: E402
from keisei_amd.sl.dataset import write_shard  # noqa: E402
from oracle.shogi import OracleVecEnv  # noqa: E402


def synthetic_games(n: int, moves: int, seed: int = 0):
    """n oracle playouts as (action indices, outcome, host reason)."""
    rng = np.random.default_rng(seed)
    want = rng.integers(moves * 3 // 4, moves * 5 // 4 + 1, n)
    env = OracleVecEnv(n, 65535)
    _, mask = env.reset()
    acts, alive = [[] for _ in range(n)], np.ones(n, bool)
    for i in range(int(want.max())):
        pick = np.array([rng.choice(np.flatnonzero(m)) for m in mask], dtype=np.int64)
        for e in np.flatnonzero(alive & (i < want)):
            acts[e].append(int(pick[e]))
        r = env.step(pick)
        alive &= ~(r["terminated"] | r["truncated"])
        mask = r["legal_masks"]
    return [(np.asarray(a, np.int32), int(rng.integers(0, 3)), prep.REASON_NONE) for a in acts]


def timed(fn, repeat: int):
    fn()                                                        # warm-up
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
    ap.add_argument("--games", type=int, default=512)
    ap.add_argument("--moves", type=int, default=120)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--shard-size", type=int, default=100_000)
    args = ap.parse_args()
    games = synthetic_games(args.games, args.moves)
    max_moves = max(len(g[0]) for g in games)
    batch = prep.ReplayBatch.build(games)
    dev = prep._DeviceReplay(args.games, max_moves)
    host_env = VecEnv(args.games, max_moves, "katago", "spatial", output="numpy")
    seen = {}

    def device_batch():
        buf, valid_len, reason, hdr = dev.replay(batch)
        seen["dev"] = (buf[prep._kept_rows(batch, valid_len)], hdr)
        return seen["dev"][0]

    def host_batch():
        buf, valid_len, reason, hdr = prep._replay_host(batch, host_env)
        seen["host"] = (buf[prep._kept_rows(batch, valid_len)], hdr)
        return seen["host"][0]

    def device_files():
        with tempfile.TemporaryDirectory() as d:
            w = prep._ShardWriter(Path(d), args.shard_size)
            w.append(device_batch())
            w.close()

    def host_files():                                           # the writer the package had: write_shard per shard
        with tempfile.TemporaryDirectory() as d:
            rec = host_batch()
            for k, at in enumerate(range(0, len(rec), args.shard_size)):
                part = rec[at:at + args.shard_size]
                write_shard(Path(d) / f"shard_{k:03d}.bin", part["obs"], part["policy"], part["value"], part["score"])

    t = {name: timed(fn, args.repeat) for name, fn in (("device", device_batch), ("device_files", device_files),
                                                      ("host", host_batch), ("host_files", host_files))}
    same = seen["dev"][0].tobytes() == seen["host"][0].tobytes()
    n, hdr = len(seen["dev"][0]), seen["dev"][1]
    steps = int(hdr[prep._WRITTEN] + hdr[prep._FILLER])
    print(json.dumps({
        "metric": "sl_prepare_positions_per_s", "games": args.games, "positions": n, "plies": int(hdr[prep._PLIES]),
        "filler_share": round(int(hdr[prep._FILLER]) / steps, 4), "records_equal_host_path": same,
        "device_pos_per_s": round(n / t["device"]), "device_with_files_pos_per_s": round(n / t["device_files"]),
        "host_pos_per_s": round(n / t["host"]), "host_with_files_pos_per_s": round(n / t["host_files"]),
        "ratio": round(t["host"] / t["device"], 2), "ratio_with_files": round(t["host_files"] / t["device_files"], 2),
        "device_s": round(t["device"], 4), "host_s": round(t["host"], 4), "repeat": args.repeat}))


if __name__ == "__main__":
    main()
