"""LeagueRollout (the learner-vs-league rollout epoch on the device, host read every sync_every plies) against a host
loop built from what the package offered before it: split_merge_step + the device PendingTransitions + buffer.add on
the device VecEnv, with the done handling of the reference (katago_loop.py:1376-1437) on the host.

  (a) b10c128, learner + 7 opponents, 512 envs
  (b) 40x256, learner + 3 opponents, 256 envs

Every config runs one epoch of --steps plies after one warm-up epoch (kernel loading, graph capture, buffer growth) and
reports plies/s (epoch plies over wall time), rows/s and host syncs (LeagueRollout counts its state reads; the host
loop's figure is a tally kept by hand where it is known to read from the device).  Both sides re-draw colours.  Clocks are not pinned.  One JSON line per workload.

    python tools/league_bench.py [--workload a|b|all] [--configs g32,e2,host] [--steps 128] [--max-ply 512] [--repeat 1]
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

from keisei_amd.shogi_gym import ACTION_SPACE, VecEnv  # noqa: E402
from keisei_amd.training import LeagueRollout  # noqa: E402
from keisei_amd.training.katago_loop import (PendingTransitions, _compute_value_cats, _resolve_opponent_devices,  # noqa: E402
                                             sign_correct_bootstrap, split_merge_step, to_learner_perspective)
from keisei_amd.training.katago_ppo import KataGoRolloutBuffer  # noqa: E402
from keisei_amd.training.models.se_resnet import SEResNetModel, SEResNetParams  # noqa: E402
from keisei_amd.training.value_adapter import MultiHeadValueAdapter  # noqa: E402
from oracle import keisei_oracle as orc  # noqa: E402

WORKLOADS = {"a": ("b10c128_k8", orc.NetShape(10, 128, 8, 64, 16, 128, 64), 8, 512),
             "b": ("40x256_k4", orc.NetShape(), 4, 256)}
CONFIGS = {"g32": (True, 32), "g2": (True, 2), "e2": (False, 2), "e32": (False, 32)}
OBS = (50, 9, 9)


def _models(shape, K):
    ms = []
    for k in range(K):
        m = SEResNetModel(SEResNetParams(**shape.__dict__))
        m.load_state_dict(orc.init_like_state_dict(shape, salt=13 * k + 1), strict=True)
        ms.append(m.to("cuda").eval())
    return ms


def host_loop_epoch(models, env, buffer, steps, state, adapter, score_norm=76.0):
    """the reference's opponent branch (katago_loop.py:1162-1437, :1537-1563) with this package's helpers; `state` carries
    the players, the per-env opponents and the generator from one epoch to the next, as the reference's loop does"""
    N, dev = env.num_envs, env.device
    learner, cohort = models[0], {k: m for k, m in enumerate(models[1:])}
    devices = _resolve_opponent_devices(cohort, dev)
    pending = PendingTransitions(N, OBS, ACTION_SPACE, dev)
    rng, opp_ids, players = state["rng"], state["opp"], state["players"]
    learner_side = rng.integers(0, 2, N).astype(np.uint8)          # :1134-1137: all sides anew every epoch
    results = {k: [0, 0, 0] for k in cohort}
    syncs = 0          # a tally kept by hand at the places known to read from the device, not a measurement
    t0 = time.monotonic()
    for _ in range(steps):
        cur = env.current()
        obs, bits = cur.observations, cur.legal_mask_bits
        pre = players.copy()
        sm = split_merge_step(obs, bits, players, learner, opponent_models=cohort, env_opponent_ids=opp_ids,
                              learner_side=learner_side, value_adapter=adapter, opponent_devices=devices)
        syncs += 1 + 1 + len(cohort)                             # group sizes, the learner's draw, one draw per opponent with rows
        r = env.step(sm.actions)
        players = r.current_players.cpu().numpy()
        syncs += 1
        learner_next = torch.from_numpy(players == learner_side).to(dev)
        learner_moved = torch.from_numpy(pre == learner_side).to(dev)
        dones = r.terminated | r.truncated
        learner_rewards = to_learner_perspective(r.rewards, pre, learner_side)
        truncated_only = r.truncated & ~r.terminated
        override = None
        if bool(truncated_only.any()):
            with torch.no_grad():
                out = learner(r.terminal_observations)
            tv = sign_correct_bootstrap(adapter.scalar_value_blended(out.value_logits.float(), out.score_lead.float()),
                                        1 - pre, learner_side)
            override = torch.full_like(tv, float("nan"))
            override[truncated_only] = tv[truncated_only]
        syncs += 1
        pending.accumulate_reward(learner_rewards)
        fin = pending.finalize(pending.valid & (dones | learner_next), dones, r.terminated)
        syncs += 1
        if fin is not None:
            buffer.add(fin["obs"], fin["actions"], fin["log_probs"], fin["values"], fin["rewards"], fin["dones"],
                       fin["terminated"], fin["legal_mask_bits"], _compute_value_cats(fin["rewards"], fin["terminated"].bool(), dev),
                       fin["score_targets"], env_ids=fin["env_ids"],
                       next_value_override=override[fin["env_ids"]] if override is not None else None)
            syncs += 1
        if bool(learner_moved.any()):
            lp, vals = torch.zeros(N, device=dev), torch.zeros(N, device=dev)
            lp[sm.learner_indices], vals[sm.learner_indices] = sm.learner_log_probs.float(), sm.learner_values.float()
            pending.create(learner_moved, obs, sm.actions, lp, vals, bits, learner_rewards,
                           r.step_metadata.material_balance.float() / score_norm)
            imm = learner_moved & dones
            if bool(imm.any()):
                fin = pending.finalize(imm, dones, r.terminated)
                if fin is not None:
                    buffer.add(fin["obs"], fin["actions"], fin["log_probs"], fin["values"], fin["rewards"], fin["dones"],
                               fin["terminated"], fin["legal_mask_bits"],
                               _compute_value_cats(fin["rewards"], fin["terminated"].bool(), dev), fin["score_targets"],
                               env_ids=fin["env_ids"], next_value_override=override[fin["env_ids"]] if override is not None else None)
                    syncs += 1
            syncs += 2
        if bool(dones.any()):                                    # :1376-1437 on the host
            done_np = dones.cpu().numpy()
            idx = np.flatnonzero(done_np)
            rew = learner_rewards[dones].cpu().numpy()
            term = r.terminated.cpu().numpy()[idx]
            for i, e in enumerate(idx):
                if term[i]:
                    results[int(opp_ids[e])][0 if rew[i] > 0 else (1 if rew[i] < 0 else 2)] += 1
                opp_ids[e] = rng.integers(0, len(cohort))
            learner_side[done_np] = rng.integers(0, 2, int(done_np.sum())).astype(np.uint8)    # :1418-1437
        syncs += 1
    if bool(pending.valid.any()):
        z = torch.zeros(N, device=dev)
        fin = pending.finalize(pending.valid.clone(), z, z)
        if fin is not None:
            buffer.add(fin["obs"], fin["actions"], fin["log_probs"], fin["values"], fin["rewards"], fin["dones"],
                       fin["terminated"], fin["legal_mask_bits"], torch.full((fin["env_ids"].numel(),), -1, dtype=torch.long, device=dev),
                       fin["score_targets"], env_ids=fin["env_ids"])
    env.raise_if_refused()
    torch.cuda.synchronize()
    dt = time.monotonic() - t0
    state["players"] = players
    rows = buffer._write_offset
    return {"epoch_s": round(dt, 3), "plies_per_s": round(steps / dt, 1), "rows": rows, "rows_per_s": round(rows / dt, 1),
            "host_syncs_tallied_by_hand": syncs, "games": sum(sum(v) for v in results.values())}


def league_epoch(models, N, max_ply, graph, sync_every, steps, adapter, repeat):
    roll = LeagueRollout(models[0], models[1:], list(range(len(models) - 1)), num_envs=N, max_ply=max_ply, value_adapter=adapter,
                         color_randomization=True, sync_every=sync_every, graph=graph, seed=1234)
    buf = KataGoRolloutBuffer(N, OBS, ACTION_SPACE, device="cuda")
    roll.collect(buf, steps)                                     # warm-up: graph capture, buffer growth
    torch.cuda.synchronize()
    runs = []
    for _ in range(repeat):
        buf.clear()
        t0 = time.monotonic()
        st = roll.collect(buf, steps)
        torch.cuda.synchronize()
        dt = time.monotonic() - t0
        runs.append(round(steps / dt, 1))
    return {"plies_per_s_runs": runs, "epoch_s": round(dt, 3), "plies_per_s": round(steps / dt, 1), "rows": st.rows,
            "rows_per_s": round(st.rows / dt, 1), "host_syncs": st.host_syncs, "games": st.terminated + st.truncated,
            "truncation_overrides": st.truncation_overrides}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="all", choices=["a", "b", "all"])
    ap.add_argument("--configs", default="g32,e2,host")
    ap.add_argument("--steps", type=int, default=128)
    ap.add_argument("--max-ply", type=int, default=512)
    ap.add_argument("--repeat", type=int, default=1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "league_bench needs a GPU"
    adapter = MultiHeadValueAdapter()
    lines = []
    for w in (["a", "b"] if args.workload == "all" else [args.workload]):
        name, shape, K, N = WORKLOADS[w]
        models = _models(shape, K)
        row = {"workload": name, "num_envs": N, "models": K, "steps": args.steps, "max_ply": args.max_ply, "clocks": "unpinned"}
        for c in args.configs.split(","):
            if c == "host":
                env = VecEnv(N, args.max_ply, "katago", "spatial", output="torch", check_actions=False)
                env.reset()
                state = {"rng": np.random.default_rng(1), "players": np.zeros(N, np.uint8),
                         "opp": np.random.default_rng(2).integers(0, K - 1, N)}
                buf = KataGoRolloutBuffer(N, OBS, ACTION_SPACE, device="cuda")
                host_loop_epoch(models, env, buf, min(args.steps, 16), state, adapter)     # warm-up
                buf.clear()
                row["host_loop"] = host_loop_epoch(models, env, buf, args.steps, state, adapter)
            else:
                graph, se = CONFIGS[c]
                row[f"league_{'graph' if graph else 'eager'}_sync{se}"] = league_epoch(models, N, args.max_ply, graph, se,
                                                                                      args.steps, adapter, args.repeat)
            torch.cuda.synchronize()
        print(json.dumps(row), flush=True)
        lines.append(row)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(json.dumps(r) for r in lines) + "\n")


if __name__ == "__main__":
    main()
