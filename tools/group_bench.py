"""Grouped eval forward (SEResNetGroup: three launches) against the per-model loop a league caller runs today (each model's
own forward on its rows: bf16 autocast, the graph-captured eval path), at two workloads:

  (a) b10c128, 20 models, 256 boards, scattered model_idx   (keisei-500k-league: 64 matches x 4 envs over up to 22 models)
  (b) 40x256, 4 models, 128 boards

Two loop timings: 'fixed' reuses one model_idx (every model's board count repeats, so its captured graph is replayed: the
loop's best case) and 'varying' draws a new scattered model_idx per call (board counts change from ply to ply, as in league
play: new counts cost a warm-up forward and a capture).  Times are wall-clock per call around a synchronised call (the
per-model loop is host-bound), median and spread of R repeats after W warm-up calls.

    python tools/group_bench.py [--repeats 30] [--warmup 5] [--out results.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from keisei_amd.training.model_group import SEResNetGroup  # noqa: E402
from keisei_amd.training.models.se_resnet import SEResNetModel, SEResNetParams  # noqa: E402
from oracle import keisei_oracle as orc  # noqa: E402

WORKLOADS = {"a_b10c128_k20_b256": (orc.NetShape(10, 128, 8, 64, 16, 128, 64), 20, 256),
             "b_40x256_k4_b128": (orc.NetShape(), 4, 128)}


def _models(shape, K):
    out = []
    for k in range(K):
        m = SEResNetModel(SEResNetParams(**shape.__dict__))
        m.load_state_dict(orc.init_like_state_dict(shape, salt=k + 1), strict=True)
        out.append(m.to("cuda").eval())
    return out


def _loop(models, obs, idx):
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        for k, m in enumerate(models):
            rows = (idx == k).nonzero(as_tuple=True)[0]
            if rows.numel():
                m(obs[rows])


def _time(fn, warmup, repeats):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return {"median_ms": statistics.median(ts), "min_ms": ts[0], "max_ms": ts[-1], "n": repeats}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default="", help="also write the results as one JSON file here")
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "env": {k: v for k, v in os.environ.items() if k.startswith("KA_")}}
    for name, (shape, K, B) in WORKLOADS.items():
        if args.only and args.only not in name:
            continue
        models = _models(shape, K)
        grp = SEResNetGroup(models)
        g = torch.Generator().manual_seed(0)
        obs = torch.randn(B, 50, 9, 9, generator=g).cuda()
        idx = torch.randint(0, K, (B,), generator=g).cuda()
        idxs = [torch.randint(0, K, (B,), generator=g).cuda() for _ in range(args.warmup + args.repeats)]
        it = iter(idxs)
        r = {"K": K, "B": B, "shape": shape.__dict__,
             "grouped_check": _time(lambda: grp.forward(obs, idx), args.warmup, args.repeats),
             "grouped_nocheck": _time(lambda: grp.forward(obs, idx, check=False), args.warmup, args.repeats),
             "loop_fixed": _time(lambda: _loop(models, obs, idx), args.warmup, args.repeats),
             "loop_varying": _time(lambda: _loop(models, obs, next(it)), args.warmup, args.repeats)}
        # GPU time of the three grouped launches alone (events, back-to-back calls)
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        for _ in range(args.warmup):
            grp.forward(obs, idx, check=False)
        s.record()
        for _ in range(args.repeats):
            grp.forward(obs, idx, check=False)
        e.record()
        torch.cuda.synchronize()
        r["grouped_gpu_ms_per_call"] = s.elapsed_time(e) / args.repeats
        r["speedup_vs_loop_fixed"] = r["loop_fixed"]["median_ms"] / r["grouped_check"]["median_ms"]
        r["speedup_vs_loop_varying"] = r["loop_varying"]["median_ms"] / r["grouped_check"]["median_ms"]
        res[name] = r
        print(name, json.dumps(r), flush=True)
        del models, grp
        torch.cuda.empty_cache()
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
