"""MatchArena (whole ply on the device, host read every sync_every plies) against a host loop written the reference's way
(ConcurrentMatchPool.run_round, concurrent_matches.py:196-545: seat lists with nonzero on host copies of the players,
SEResNetGroup.select_actions with check=True, win / loss / draw tallies in Python), over the same group and VecEnv.

  (a) b10c128, 8 models, 16 pairings, 64 games, 512 envs / 64 per match
  (b) 40x256, 4 models, 4 pairings, 64 games, 256 envs / 64 per match

Both run one round after a warm-up round (kernel loading, graph capture) and report plies/s, games/min and host syncs per
round.  One JSON line per workload.

A config name ending in "c" (g32c, e2c, ...) builds the arena with collect=True and makes every pairing trainable on both
sides: the worst case of rollout collection, reported with the rows collected.  An "f" (g32f, and
g32cf with collection) builds it with features=True, reported with the feature rows and the time the
host spent draining game records.

    python tools/arena_bench.py [--workload a|b|all] [--configs g2,g32,e2,e32,host,g32c,g32f,g32cf] [--max-ply 512] [--repeat 1]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from keisei_amd.shogi_gym import VecEnv  # noqa: E402
from keisei_amd.training import MatchArena  # noqa: E402
from keisei_amd.training.model_group import SEResNetGroup  # noqa: E402
from keisei_amd.training.models.se_resnet import SEResNetModel, SEResNetParams  # noqa: E402
from oracle import keisei_oracle as orc  # noqa: E402

WORKLOADS = {"a": ("b10c128_k8_p16", orc.NetShape(10, 128, 8, 64, 16, 128, 64), 8, 16, 512, 64),
             "b": ("40x256_k4_p4", orc.NetShape(), 4, 4, 256, 64)}
CONFIGS = {"g2": (True, 2), "g32": (True, 32), "e2": (False, 2), "e32": (False, 32)}


def _group(shape, K):
    ms = []
    for k in range(K):
        m = SEResNetModel(SEResNetParams(**shape.__dict__))
        m.load_state_dict(orc.init_like_state_dict(shape, salt=13 * k + 1), strict=True)
        ms.append(m.to("cuda").eval())
    return SEResNetGroup(ms)


def _pairings(K, P):
    out, i = [], 0
    while len(out) < P:
        a, b = i % K, (i // K + 1 + i) % K
        if a != b:
            out.append((a, b))
        i += 1
    return out


def host_loop_round(group, env, pairings, games, max_ply, E):
    """the reference's run_round over the device VecEnv and the grouped forward, with its host-side bookkeeping"""
    N, dev = env.num_envs, env.device
    S = N // E
    syncs = 0
    t0 = time.monotonic()
    env.reset()
    players = np.zeros(N, dtype=np.uint8)
    slots = [dict(i=i, pairing=None, aw=0, bw=0, dr=0, target=games, plies=0) for i in range(min(S, len(pairings)))]
    nxt, results = 0, {}
    for s in slots:
        s["pairing"], nxt = nxt, nxt + 1
    active = list(slots)
    total_plies = 0
    while active:
        for s in active:
            s["plies"] += 1
        cur = env.current()
        model_idx = np.full(N, -1, dtype=np.int64)
        for s in active:
            lo, hi = s["i"] * E, (s["i"] + 1) * E
            a, b = pairings[s["pairing"]]
            part = players[lo:hi]
            model_idx[lo + np.nonzero(part == 0)[0]] = a
            model_idx[lo + np.nonzero(part != 0)[0]] = b
        pre = players.copy()
        idx = torch.from_numpy(model_idx).to(dev)
        actions, _ = group.select_actions(cur.observations, cur.legal_mask_bits, idx, check=True)
        syncs += 2                                           # the range check and the flags read
        first = cur.legal_masks.to(torch.long).argmax(dim=-1)   # idle partitions: first legal action
        actions = torch.where(idx >= 0, actions, first)
        r = env.step(actions)
        total_plies += 1
        rewards, term = r.rewards.cpu().numpy(), r.terminated.cpu().numpy()
        trunc, players = r.truncated.cpu().numpy(), r.current_players.cpu().numpy()
        syncs += 1                                           # (the four copies drain one stream: counted as one)
        done_pos = []
        for i, s in enumerate(active):
            lo, hi = s["i"] * E, (s["i"] + 1) * E
            done = term[lo:hi] | trunc[lo:hi]
            for k in range(hi - lo):
                if done[k]:
                    rr, a_moved = float(rewards[lo + k]), pre[lo + k] == 0
                    if rr > 0:
                        s["aw" if a_moved else "bw"] += 1
                    elif rr < 0:
                        s["bw" if a_moved else "aw"] += 1
                    else:
                        s["dr"] += 1
            if s["aw"] + s["bw"] + s["dr"] >= s["target"]:
                done_pos.append(i)
            elif s["plies"] >= max_ply * (-(-s["target"] // E) + 1):
                done_pos.append(i)
        for i in sorted(done_pos, reverse=True):
            s = active.pop(i)
            results[s["pairing"]] = (s["aw"], s["bw"], s["dr"])
            if nxt < len(pairings):
                s.update(pairing=nxt, aw=0, bw=0, dr=0, plies=0)
                nxt += 1
                active.append(s)
    env.raise_if_refused()
    dt = time.monotonic() - t0
    games_total = sum(sum(v) for v in results.values())
    return {"round_s": round(dt, 3), "round_plies": total_plies, "plies_per_s": round(total_plies / dt, 1),
            "games": games_total, "games_per_min": round(games_total / dt * 60, 1), "host_syncs": syncs}


def arena_round(group, N, E, max_ply, graph, sync_every, pairings, games, collect=False, repeat=1, features=False):
    arena = MatchArena(group, N, E, max_ply, sync_every=sync_every, graph=graph, seed=1234, collect=collect, features=features)
    drain = [0.0, 0]
    if features:                                             # time the host side of a sync point: the record drain
        inner = arena._drain_features

        def timed(*a):
            t0 = time.perf_counter()
            inner(*a)
            drain[0] += time.perf_counter() - t0
            drain[1] += 1

        arena._drain_features = timed
    kw = {"trainable": (lambda a, b: 3)} if collect else {}
    arena.run_round(pairings[:2], games_per_match=1, **kw)    # warm-up: kernel loading and graph capture
    torch.cuda.synchronize()
    rates = []
    for _ in range(repeat):
        drain[:] = [0.0, 0]
        results, st = arena.run_round(pairings, games_per_match=games, **kw)
        torch.cuda.synchronize()
        rates.append(round(st.round_plies / st.round_duration_s, 1))
    dt = st.round_duration_s
    extra = {"feature_rows": st.feature_rows, "features_dropped": st.features_dropped,
             "drain_us_per_sync": round(drain[0] / max(1, drain[1]) * 1e6, 1)} if features else {}
    return {**extra, "plies_per_s_runs": rates, "rollout_rows": st.rollout_rows, "rollouts_dropped": st.rollouts_dropped,
            "round_s": round(dt, 3), "round_plies": st.round_plies, "plies_per_s": round(st.round_plies / dt, 1),
            "games": st.total_games, "games_per_min": round(st.total_games / dt * 60, 1), "host_syncs": st.host_syncs,
            "partial": sum(r.partial for r in results),
            "a_b_d": [sum(r.a_wins for r in results), sum(r.b_wins for r in results), sum(r.draws for r in results)]}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="all", choices=["a", "b", "all"])
    ap.add_argument("--configs", default="g2,g32,e2,e32,host")
    ap.add_argument("--max-ply", type=int, default=512)
    ap.add_argument("--repeat", type=int, default=1, help="timed rounds per arena config")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "arena_bench needs a GPU"
    lines = []
    for w in (["a", "b"] if args.workload == "all" else [args.workload]):
        name, shape, K, P, N, E = WORKLOADS[w]
        group = _group(shape, K)
        pairings = _pairings(K, P)
        row = {"workload": name, "num_envs": N, "envs_per_match": E, "models": K, "pairings": P, "games_per_match": 64,
               "max_ply": args.max_ply}
        for c in args.configs.split(","):
            if c == "host":
                env = VecEnv(N, args.max_ply, "katago", "spatial", output="torch", check_actions=False)
                host_loop_round(group, env, pairings[:1], 1, args.max_ply, E)          # warm-up
                row["host_loop"] = host_loop_round(group, env, pairings, 64, args.max_ply, E)
            else:
                features = c.endswith("f")
                base = c[:-1] if features else c
                collect = base.endswith("c")
                graph, se = CONFIGS[base[:-1] if collect else base]
                key = f"arena_{'graph' if graph else 'eager'}_sync{se}{'_collect' if collect else ''}{'_features' if features else ''}"
                while key in row:                                # the same config named twice: alternating runs
                    key += "'"
                row[key] = arena_round(group, N, E, args.max_ply, graph, se, pairings, 64, collect, args.repeat, features)
            torch.cuda.synchronize()
        print(json.dumps(row), flush=True)
        lines.append(row)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(json.dumps(r) for r in lines) + "\n")


if __name__ == "__main__":
    main()
