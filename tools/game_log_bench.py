"""What the game log costs a rollout epoch: SelfPlayRollout.collect (``--owner selfplay``, the default) or
LeagueRollout.collect (``--owner league``: the learner against ``--opponents`` models of its own shape, colour
randomisation on) timed with and without ``game_log``.

The flagship rollout: the 40x256 learner, 512 envs, max_ply 500, sync_every 32, graph=True, 512 plies per timed collect
after one warm-up collect (kernel loading, graph capture, buffer growth).  Every variant of ``--game-log`` gets a rollout
of its own in ONE process and the timed collects alternate between them, ``--repeat`` rounds, so that a drift of the
clocks or of the host's other load falls on all variants alike.  A collect ends in a device synchronise; the time is the
host clock around it.  One JSON line: per variant the ms per ply of every round, their median and their spread
(max - min over the median); with the log on also the games drained and dropped.

``--game-log none`` builds the rollout without the keyword: the same script then runs on a tree from before the game log
(``--root`` names the tree whose ``keisei_amd`` is imported), which gives the parent's figure for the same workload.

    python tools/game_log_bench.py [--owner selfplay|league] [--game-log 0,1024] [--repeat 3] [--steps 512] [--root TREE]
                                   [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import statistics
import sys
import time
from pathlib import Path


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--game-log", default="0,1024", help="comma list of capacities; 'none' = do not pass the keyword")
    ap.add_argument("--owner", choices=("selfplay", "league"), default="selfplay")
    ap.add_argument("--opponents", type=int, default=3, help="the league's cohort size")
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--steps", type=int, default=512)
    ap.add_argument("--envs", type=int, default=512)
    ap.add_argument("--max-ply", type=int, default=500)
    ap.add_argument("--sync-every", type=int, default=32)
    ap.add_argument("--blocks", type=int, default=40)
    ap.add_argument("--channels", type=int, default=256)
    ap.add_argument("--root", default=str(Path(__file__).resolve().parent.parent))
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, args.root)

    import torch

    from keisei_amd.shogi_gym import ACTION_SPACE
    from keisei_amd.training import LeagueRollout, SelfPlayRollout
    from keisei_amd.training.katago_ppo import KataGoRolloutBuffer
    from keisei_amd.training.models.se_resnet import SEResNetModel, SEResNetParams
    from oracle import keisei_oracle as orc

    assert torch.cuda.is_available(), "game_log_bench needs a GPU"
    shape = orc.NetShape(args.blocks, args.channels)

    def net(salt):
        m = SEResNetModel(SEResNetParams(**shape.__dict__))
        m.load_state_dict(orc.init_like_state_dict(shape, salt=salt), strict=True)
        return m.to("cuda").eval()

    model = net(1)
    league = args.owner == "league"
    cohort = [net(2 + k) for k in range(args.opponents)] if league else []
    variants = args.game_log.split(",")
    rolls = {}
    for v in variants:
        kw = {} if v == "none" else {"game_log": int(v)}
        if league:
            rolls[v] = LeagueRollout(model, cohort, list(range(1, args.opponents + 1)), num_envs=args.envs, max_ply=args.max_ply,
                                     sync_every=args.sync_every, graph=True, seed=1234, color_randomization=True, **kw)
        else:
            rolls[v] = SelfPlayRollout(model, num_envs=args.envs, max_ply=args.max_ply, sync_every=args.sync_every, graph=True,
                                       seed=1234, **kw)
    buf = KataGoRolloutBuffer(args.envs, (50, 9, 9), ACTION_SPACE, device="cuda")
    for roll in rolls.values():                                  # warm-up: graph capture, buffer growth
        buf.clear()
        roll.collect(buf, args.steps)
    torch.cuda.synchronize()
    ms = {v: [] for v in variants}
    games = {v: [0, 0] for v in variants}
    for _ in range(args.repeat):
        for v, roll in rolls.items():
            buf.clear()
            torch.cuda.synchronize()
            t0 = time.monotonic()
            st = roll.collect(buf, args.steps)
            torch.cuda.synchronize()
            ms[v].append(round(1e3 * (time.monotonic() - t0) / args.steps, 4))
            games[v][0] += len(getattr(st, "games", []))
            games[v][1] += getattr(st, "games_dropped", 0)
    row = {"metric": f"{args.owner}_collect_ms_per_ply", "label": args.label, "envs": args.envs, "max_ply": args.max_ply,
           "sync_every": args.sync_every, "steps": args.steps, "net": f"{args.blocks}x{args.channels}", "clocks": "unpinned"}
    if league:
        row["opponents"] = args.opponents
    for v in variants:
        med = statistics.median(ms[v])
        row[f"game_log_{v}"] = {"ms_per_ply_runs": ms[v], "median": round(med, 4),
                                "spread": round((max(ms[v]) - min(ms[v])) / med, 4), "games": games[v][0], "dropped": games[v][1]}
    line = json.dumps(row)
    print(line, flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
