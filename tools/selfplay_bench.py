"""SelfPlayRollout (the self-play rollout epoch on the device, host read every sync_every plies) against the host loop it
replaces: KataGoPPOAlgorithm.select_actions + VecEnv.step + the bookkeeping of the reference's no-opponent branch
(katago_loop.py:1453-1527) on device tensors + buffer.add, one ply at a time from Python.

  (a) b10c128, 512 envs, 128 plies
  (b) 40x256, 256 envs, 64 plies

Every config runs --repeat epochs after one warm-up epoch (kernel loading, graph capture, buffer growth) and reports
plies/s (epoch plies over wall time), rows/s, ms per ply and host syncs (SelfPlayRollout counts its state reads; the host
loop's figure is a tally kept by hand where it is known to read from the device).  Clocks are not pinned.  One JSON line
per workload.

--move-history runs every device config a second time with SelfPlayRollout(move_history=True) (the env then keeps the move
notes of the games in progress: two more launches per ply) under the key suffix "_hist", and times one spectator_data()
call over all envs behind each device config's last epoch ("spectator_data_ms").

--insight K runs every device config once more with SelfPlayRollout(insight=K) (the policy insight of every move: one
more launch per ply, ka_policy_insight) under the key suffix "_insight"; with --move-history the "_hist" run carries the
switch as well (the per-move records are then kept), under "_hist_insight".

    python tools/selfplay_bench.py [--workload a|b|all] [--configs g32,e2,host] [--steps N] [--max-ply 512] [--repeat 2]
                                   [--move-history] [--insight K]
"""
from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import torch  # noqa: E402

from keisei_amd.shogi_gym import ACTION_SPACE, VecEnv  # noqa: E402
from keisei_amd.training import SelfPlayRollout  # noqa: E402
from keisei_amd.training.katago_loop import _compute_value_cats  # noqa: E402
from keisei_amd.training.katago_ppo import KataGoPPOAlgorithm, KataGoPPOParams, KataGoRolloutBuffer  # noqa: E402
from keisei_amd.training.models.se_resnet import SEResNetModel, SEResNetParams  # noqa: E402
from keisei_amd.training.value_adapter import MultiHeadValueAdapter  # noqa: E402
from oracle import keisei_oracle as orc  # noqa: E402

WORKLOADS = {"a": ("b10c128", orc.NetShape(10, 128, 8, 64, 16, 128, 64), 512, 128),
             "b": ("40x256", orc.NetShape(), 256, 64)}
CONFIGS = {"g32": (True, 32), "g2": (True, 2), "e2": (False, 2), "e32": (False, 32)}
OBS = (50, 9, 9)


def _model(shape):
    m = SEResNetModel(SEResNetParams(**shape.__dict__))
    m.load_state_dict(orc.init_like_state_dict(shape, salt=1), strict=True)
    return m.to("cuda")


def host_loop_epoch(ppo, env, buffer, steps, adapter, score_norm=76.0):
    """the reference's no-opponent branch (katago_loop.py:1441-1527, :1565-1590), one ply at a time"""
    dev = env.device
    model = ppo.forward_model
    tallies = torch.zeros(7, dtype=torch.int64, device=dev)    # wins, losses, draws, black, white, terminated, truncated
    syncs = 0          # a tally kept by hand at the places known to read from the device, not a measurement
    t0 = time.monotonic()
    players = env._players[env._cur]
    for _ in range(steps):
        cur = env.current()
        obs, masks = cur.observations, cur.legal_masks
        with torch.no_grad():
            actions, log_probs, values = ppo.select_actions(obs, masks, value_adapter=adapter)
        syncs += 1                                               # the sampler's flags
        pre = players
        r = env.step(actions)
        players = r.current_players
        rewards, terminated, truncated = r.rewards, r.terminated, r.truncated
        dones = terminated | truncated
        tallies[5] += terminated.sum()
        tallies[6] += (truncated & ~terminated).sum()
        if bool(terminated.any()):
            tr, who = rewards[terminated], pre[terminated]
            tallies[0] += (tr > 0).sum(); tallies[1] += (tr < 0).sum(); tallies[2] += (tr == 0).sum()
            tallies[3] += (((tr > 0) & (who == 0)) | ((tr < 0) & (who == 1))).sum()
            tallies[4] += (((tr > 0) & (who == 1)) | ((tr < 0) & (who == 0))).sum()
        syncs += 1
        cats = _compute_value_cats(rewards, terminated, dev)
        score_targets = r.step_metadata.material_balance.float() / score_norm
        truncated_only = truncated & ~terminated
        override = None
        if bool(truncated_only.any()):
            model.eval()
            with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
                out = model(r.terminal_observations)
            model.train()
            tv = adapter.scalar_value_blended(out.value_logits.float(), out.score_lead.float())
            override = torch.full_like(tv, float("nan"))
            override[truncated_only] = -tv[truncated_only]
        syncs += 1
        buffer.add(obs, actions, log_probs, values, rewards, dones, terminated, masks, cats, score_targets,
                   next_value_override=override)
        syncs += 1                                               # the store's guard flags
    model.eval()
    with torch.no_grad(), torch.autocast("cuda", dtype=torch.bfloat16):
        out = model(env.current().observations)
    model.train()
    next_values = -adapter.scalar_value_blended(out.value_logits.float(), out.score_lead.float())
    buffer.fill_alternating_perspective_overrides()
    env.raise_if_refused()
    torch.cuda.synchronize()
    dt = time.monotonic() - t0
    rows = buffer._write_offset
    t = tallies.tolist()
    return {"epoch_s": round(dt, 3), "plies_per_s": round(steps / dt, 1), "ms_per_ply": round(1e3 * dt / steps, 3), "rows": rows,
            "rows_per_s": round(rows / dt, 1), "host_syncs_tallied_by_hand": syncs, "games": t[5] + t[6],
            "next_values_finite": bool(torch.isfinite(next_values).all())}


def device_epochs(model, N, max_ply, graph, sync_every, steps, adapter, repeat, move_history=False, feed=False, insight=0):
    extra = {"insight": insight} if insight else {}              # (nothing new is passed where the switch is off)
    roll = SelfPlayRollout(model, num_envs=N, max_ply=max_ply, value_adapter=adapter, sync_every=sync_every, graph=graph,
                           seed=1234, move_history=move_history, **extra)
    buf = KataGoRolloutBuffer(N, OBS, ACTION_SPACE, device="cuda")
    roll.collect(buf, steps)                                     # warm-up: graph capture, buffer growth
    roll.bootstrap_values()
    torch.cuda.synchronize()
    runs = []
    for _ in range(repeat):
        buf.clear()
        t0 = time.monotonic()
        st = roll.collect(buf, steps)
        roll.bootstrap_values()
        torch.cuda.synchronize()
        dt = time.monotonic() - t0
        runs.append(round(steps / dt, 1))
    out = {"plies_per_s_runs": runs, "epoch_s": round(dt, 3), "plies_per_s": round(steps / dt, 1),
           "ms_per_ply": round(1e3 * dt / steps, 3), "rows": st.rows, "rows_per_s": round(st.rows / dt, 1),
           "host_syncs": st.host_syncs, "games": st.terminated + st.truncated, "truncation_overrides": st.truncation_overrides}
    if feed:
        t0 = time.monotonic()
        data = roll.spectator_data()
        out["spectator_data_ms"] = round(1e3 * (time.monotonic() - t0), 2)
        out["history_moves"] = sum(len(d["move_history"]) for d in data)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="all", choices=["a", "b", "all"])
    ap.add_argument("--configs", default="g32,e2,host")
    ap.add_argument("--steps", type=int, default=None, help="plies per epoch (default: the workload's)")
    ap.add_argument("--max-ply", type=int, default=512)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--move-history", action="store_true", help="also run the device configs with move_history=True")
    ap.add_argument("--insight", type=int, default=0, help="also run the device configs with insight=K (top_k of the policy insight)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "selfplay_bench needs a GPU"
    adapter = MultiHeadValueAdapter()
    lines = []
    for w in (["a", "b"] if args.workload == "all" else [args.workload]):
        name, shape, N, steps = WORKLOADS[w]
        steps = args.steps or steps
        row = {"workload": name, "num_envs": N, "steps": steps, "max_ply": args.max_ply, "repeat": args.repeat, "clocks": "unpinned"}
        for c in args.configs.split(","):
            model = _model(shape)                                # a model of its own per config: no config inherits a mode
            if c == "host":
                model.train()                                    # the training loop's mode between select_actions calls
                ppo = KataGoPPOAlgorithm(KataGoPPOParams(batch_size=4096, use_amp=True), model)
                env = VecEnv(N, args.max_ply, "katago", "spatial", output="torch", check_actions=False)
                env.reset()
                buf = KataGoRolloutBuffer(N, OBS, ACTION_SPACE, device="cuda")
                host_loop_epoch(ppo, env, buf, min(steps, 16), adapter)      # warm-up
                runs = []
                for _ in range(args.repeat):
                    buf.clear()
                    res = host_loop_epoch(ppo, env, buf, steps, adapter)
                    runs.append(res["plies_per_s"])
                row["host_loop"] = dict(res, plies_per_s_runs=runs)
            else:
                graph, se = CONFIGS[c]
                key = f"selfplay_{'graph' if graph else 'eager'}_sync{se}"
                row[key] = device_epochs(model.eval(), N, args.max_ply, graph, se, steps, adapter, args.repeat,
                                         feed=args.move_history)
                if args.move_history:
                    row[key + "_hist"] = device_epochs(_model(shape).eval(), N, args.max_ply, graph, se, steps, adapter,
                                                       args.repeat, move_history=True, feed=True)
                if args.insight:
                    row[key + "_insight"] = device_epochs(_model(shape).eval(), N, args.max_ply, graph, se, steps, adapter,
                                                          args.repeat, feed=True, insight=args.insight)
                    if args.move_history:
                        row[key + "_hist_insight"] = device_epochs(_model(shape).eval(), N, args.max_ply, graph, se, steps, adapter,
                                                                   args.repeat, move_history=True, feed=True, insight=args.insight)
            torch.cuda.synchronize()
        print(json.dumps(row), flush=True)
        lines.append(row)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text("\n".join(json.dumps(r) for r in lines) + "\n")


if __name__ == "__main__":
    main()
