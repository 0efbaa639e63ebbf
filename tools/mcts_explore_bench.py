"""What exploration costs a searched arena ply: times MatchArena.run_round with mcts= at 256 envs, width 8 and
16 simulations, two 6 x 128 SE-ResNets, a warm round and then ``--rounds`` timed rounds, one JSON line per round.

    python tools/mcts_explore_bench.py [--root TREE] [--mode absent|off|on] [--tag NAME]

``--root`` is the checkout to import from (default: this one; the parent commit's tree for the comparison, mode ``absent``),
``--mode``: ``absent`` = no mcts_explore= argument, ``off`` = an all-off table (the launches enqueued, nothing drawn),
``on`` = epsilon 0.25, alpha 0.15, 30 plies.  Run the variants in processes of their own, alternating, on one GPU."""
import argparse
import json
import sys
import time
from pathlib import Path

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=str(Path(__file__).resolve().parent.parent))
ap.add_argument("--mode", choices=("absent", "off", "on"), default="absent")
ap.add_argument("--tag", default="")
ap.add_argument("--rounds", type=int, default=3)
args = ap.parse_args()
sys.path.insert(0, args.root)

import torch  # noqa: E402

from keisei_amd.training import MatchArena, MctsControls  # noqa: E402
from keisei_amd.training.model_group import SEResNetGroup  # noqa: E402
from keisei_amd.training.models.se_resnet import SEResNetModel, SEResNetParams  # noqa: E402
from oracle import keisei_oracle as orc  # noqa: E402

shape = orc.NetShape(6, 128, 16, 128, 32, 256, 128)
models = []
for i in range(2):
    m = SEResNetModel(SEResNetParams(**shape.__dict__))
    m.load_state_dict(orc.init_like_state_dict(shape, salt=31 * i + 7), strict=True)
    models.append(m.to("cuda").eval())
kw = {}
if args.mode != "absent":
    from keisei_amd.training import MctsExploration  # noqa: E402
    kw["mcts_explore"] = MctsExploration(0.25, 0.15, 30) if args.mode == "on" else MctsExploration.OFF
arena = MatchArena(SEResNetGroup(models), 256, 64, 64, sync_every=8, graph=True, seed=11, mcts=MctsControls(8, 16, 1.25), **kw)
pairings = [(0, 1), (1, 0), (0, 1), (1, 0)]
arena.run_round(pairings, games_per_match=64)                 # capture and warm-up
for r in range(args.rounds):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    results, stats = arena.run_round(pairings, games_per_match=64)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps(dict(tag=args.tag or args.mode, mode=args.mode, round=r, seconds=round(dt, 4), plies=stats.round_plies,
                          ms_per_ply=round(1e3 * dt / stats.round_plies, 4), searched=stats.mcts.searched,
                          noised=getattr(stats.mcts, "noised", None), sampled=getattr(stats.mcts, "sampled", None))), flush=True)
