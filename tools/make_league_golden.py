"""Generates tests/golden/g13_league_rollout.npz: the reference's learner-vs-league rollout protocol over a synthetic
stream of step results (dev container only: imports the reference tree named by KEISEI_REFERENCE; copies none of its code).

The reference's own ``PendingTransitions``, ``to_learner_perspective``, ``sign_correct_bootstrap``, ``_compute_value_cats``
and ``KataGoRolloutBuffer`` are driven in the order of katago_loop.py:1219-1365 and :1537-1563 over T plies of E envs with
a small observation shape and action space.  The stream is env facts only (movers, rewards, flags, material); the
learner's sides and the per-env opponents follow this package's draw function, which is what ``LeagueRollout`` uses on
the device.  The fixture holds the stream, the reference's flattened buffer columns (``env_ids`` and
``next_value_override`` included), ``buffer.size`` and the tallies.

The stream is searched over generator seeds until it reaches every branch of the protocol (asserted below): a learner
move that ends the game, an opponent reply that ends it, truncation on either mover, a draw, both learner colours, an
env that is done on consecutive plies, a pending row left at the end, a ply with no learner move and one with no
opponent move.

    python tools/make_league_golden.py [--out tests/golden/g13_league_rollout.npz]
"""
from __future__ import annotations

import argparse
import importlib
import os
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
REF = Path(os.environ.get("KEISEI_REFERENCE", "/root/reference"))
sys.path.insert(0, str(ROOT))
sys.dont_write_bytecode = True

from keisei_amd.training.league_rollout import cum_thresholds, draw_opponents, draw_sides  # noqa: E402

E, T, OBS_SHAPE, A = 4, 48, (2, 3, 3), 40
MAX_PLY = 6
OPPONENT_IDS = (11, 5, 23)
WEIGHTS = (1.0, 2.0, 1.0)
SCORE_NORM = 76.0
DRAW_SEED = 20240613


def make_stream(gen_seed: int) -> dict:
    """T plies of env facts: the players alternate inside a game, a game ends by a random result or at MAX_PLY plies,
    and the env starts the next game with player 0 to move."""
    g = np.random.default_rng(gen_seed)
    player, ply = np.zeros(E, np.uint8), np.zeros(E, np.int64)
    s = {k: [] for k in ("obs", "legal_masks", "pre_players", "actions", "log_probs", "values", "rewards", "terminated",
                         "truncated", "current_players", "material", "term_values")}
    for _ in range(T):
        masks = g.random((E, A)) < 0.3
        actions = g.integers(0, A, E)
        masks[np.arange(E), actions] = True
        ends = g.random(E) < 0.22
        result = g.choice(np.array([1.0, -1.0, 0.0], np.float32), E, p=[0.5, 0.25, 0.25])
        ply = ply + 1
        terminated = ends
        truncated = ~ends & (ply >= MAX_PLY)
        done = terminated | truncated
        s["obs"].append(g.random((E, *OBS_SHAPE)).astype(np.float32))
        s["legal_masks"].append(masks)
        s["pre_players"].append(player.copy())
        s["actions"].append(actions.astype(np.int64))
        s["log_probs"].append(-g.random(E).astype(np.float32) * 3)
        s["values"].append((g.random(E).astype(np.float32) * 2 - 1))
        s["rewards"].append(np.where(terminated, result, 0.0).astype(np.float32))
        s["terminated"].append(terminated.copy())
        s["truncated"].append(truncated.copy())
        s["material"].append(g.integers(-60, 61, E).astype(np.int32))
        s["term_values"].append(np.where(truncated, g.random(E) * 2 - 1, np.nan).astype(np.float32))
        player = np.where(done, 0, 1 - player).astype(np.uint8)
        ply = np.where(done, 0, ply)
        s["current_players"].append(player.copy())
    return {k: np.stack(v) for k, v in s.items()}


def run_reference(s: dict, side0: np.ndarray, opp0: np.ndarray, cum: np.ndarray):
    loop = importlib.import_module("keisei.training.katago_loop")
    ppo = importlib.import_module("keisei.training.katago_ppo")
    dev = torch.device("cpu")
    pending = loop.PendingTransitions(E, OBS_SHAPE, A, dev)
    buffer = ppo.KataGoRolloutBuffer(E, OBS_SHAPE, A)
    side, opp, games = side0.copy(), opp0.copy(), np.zeros(E, np.int64)
    tally = dict(wins=0, losses=0, draws=0, black_wins=0, white_wins=0, terminated=0, truncated=0, truncation_overrides=0)
    results = {oid: [0, 0, 0] for oid in OPPONENT_IDS}
    seen = set()
    envs = np.arange(E)
    last_done = np.zeros(E, bool)

    def add(fin, override_full, kind):
        cats = loop._compute_value_cats(fin["rewards"], fin["terminated"].bool(), dev)
        ov = override_full[fin["env_ids"]] if override_full is not None else None
        if ov is not None:
            tally["truncation_overrides"] += int((~torch.isnan(ov)).sum())
        buffer.add(fin["obs"], fin["actions"], fin["log_probs"], fin["values"], fin["rewards"], fin["dones"],
                   fin["terminated"], fin["legal_masks"], cats, fin["score_targets"], env_ids=fin["env_ids"],
                   next_value_override=ov)
        if bool(fin["dones"].any()):
            seen.add(kind + "_ends")
        if bool((fin["dones"].bool() & ~fin["terminated"].bool()).any()):
            seen.add(kind + "_truncates")

    for t in range(T):
        pre, cur = s["pre_players"][t], s["current_players"][t]
        learner_moved, learner_next = torch.from_numpy(pre == side), torch.from_numpy(cur == side)
        rewards = torch.from_numpy(s["rewards"][t])
        terminated, truncated = torch.from_numpy(s["terminated"][t]), torch.from_numpy(s["truncated"][t])
        dones = terminated | truncated
        seen.update("side%d" % v for v in side)
        if not learner_moved.any():
            seen.add("no_learner_move")
        if learner_moved.all():
            seen.add("no_opponent_move")
        if (last_done & dones.numpy()).any():
            seen.add("done_twice")
        last_done = dones.numpy().copy()
        tally["terminated"] += int(terminated.sum())
        tally["truncated"] += int((truncated & ~terminated).sum())
        learner_rewards = loop.to_learner_perspective(rewards, pre, side)
        if terminated.any():
            tr = learner_rewards[terminated]
            tally["wins"] += int((tr > 0).sum()); tally["losses"] += int((tr < 0).sum()); tally["draws"] += int((tr == 0).sum())
            if bool((tr == 0).any()):
                seen.add("draw")
            raw, who = rewards[terminated], torch.from_numpy(pre)[terminated]
            tally["black_wins"] += int((((raw > 0) & (who == 0)) | ((raw < 0) & (who == 1))).sum())
            tally["white_wins"] += int((((raw > 0) & (who == 1)) | ((raw < 0) & (who == 0))).sum())
        truncated_only = truncated & ~terminated
        override_full = None
        if bool(truncated_only.any()):
            term_v = loop.sign_correct_bootstrap(torch.from_numpy(s["term_values"][t]), 1 - pre, side)
            override_full = torch.full_like(term_v, float("nan"))
            override_full[truncated_only] = term_v[truncated_only]
        pending.accumulate_reward(learner_rewards)
        fin = pending.finalize(pending.valid & (dones.bool() | learner_next), dones, terminated)
        if fin is not None:
            add(fin, override_full, "opponent")
        if learner_moved.any():
            zero = torch.zeros(E)
            pending.create(learner_moved, torch.from_numpy(s["obs"][t]), torch.from_numpy(s["actions"][t]),
                           torch.where(learner_moved, torch.from_numpy(s["log_probs"][t]), zero),
                           torch.where(learner_moved, torch.from_numpy(s["values"][t]), zero),
                           torch.from_numpy(s["legal_masks"][t]), learner_rewards,
                           torch.from_numpy(s["material"][t].astype(np.float32)) / SCORE_NORM)
            imm = learner_moved & dones.bool()
            if imm.any():
                fin = pending.finalize(imm, dones, terminated)
                if fin is not None:
                    add(fin, override_full, "learner")
        done_np = dones.numpy()
        for e in np.flatnonzero(done_np):
            if terminated[e]:
                lr = float(learner_rewards[e])
                results[OPPONENT_IDS[opp[e]]][0 if lr > 0 else (1 if lr < 0 else 2)] += 1
        if done_np.any():
            games[done_np] += 1
            opp[done_np] = draw_opponents(DRAW_SEED, envs[done_np], games[done_np], cum)
            side[done_np] = draw_sides(DRAW_SEED, envs[done_np], games[done_np])
    if pending.valid.any():
        seen.add("pending_at_end")
        fin = pending.finalize(pending.valid.clone(), torch.zeros(E), torch.zeros(E))
        buffer.add(fin["obs"], fin["actions"], fin["log_probs"], fin["values"], fin["rewards"], fin["dones"],
                   fin["terminated"], fin["legal_masks"], torch.full((fin["env_ids"].numel(),), -1, dtype=torch.long),
                   fin["score_targets"], env_ids=fin["env_ids"])
    return buffer, tally, results, seen


WANTED = {"learner_ends", "opponent_ends", "learner_truncates", "opponent_truncates", "draw", "side0", "side1", "done_twice",
          "pending_at_end", "no_learner_move", "no_opponent_move"}


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "g13_league_rollout.npz"))
    args = ap.parse_args()
    if not (REF / "keisei").is_dir():
        sys.exit(f"needs the reference tree at {REF} (dev container only)")
    sys.path.insert(0, str(REF))
    try:                                                        # py3.10: the reference's config module wants two 3.11 names
        import tomllib  # noqa: F401
    except ModuleNotFoundError:
        sys.modules["tomllib"] = importlib.import_module("tomli")
    import enum
    if not hasattr(enum, "StrEnum"):
        class StrEnum(str, enum.Enum):
            def __str__(self) -> str:
                return str(self.value)

        enum.StrEnum = StrEnum
    cum = cum_thresholds(WEIGHTS, len(OPPONENT_IDS))
    envs = np.arange(E)
    side0 = draw_sides(DRAW_SEED, envs, np.zeros(E, np.int64))
    opp0 = draw_opponents(DRAW_SEED, envs, np.zeros(E, np.int64), cum)
    for gen_seed in range(2000):
        s = make_stream(gen_seed)
        buffer, tally, results, seen = run_reference(s, side0, opp0, cum)
        if WANTED <= seen:
            break
    else:
        raise SystemExit("no stream seed reaches every branch")
    cols = buffer.flatten()
    assert "env_ids" in cols and "next_value_override" in cols
    out = {"stream_" + k: v for k, v in s.items()}
    out.update({"col_" + k: v.numpy() for k, v in cols.items()})
    out.update(size=np.int64(buffer.size), gen_seed=np.int64(gen_seed), draw_seed=np.int64(DRAW_SEED), cum=cum, side0=side0,
               opp0=opp0, opponent_ids=np.array(OPPONENT_IDS, np.int64), weights=np.array(WEIGHTS), score_norm=np.float64(SCORE_NORM),
               obs_shape=np.array(OBS_SHAPE, np.int64), action_space=np.int64(A),
               opponent_results=np.array([results[o] for o in OPPONENT_IDS], np.int64),
               **{"tally_" + k: np.int64(v) for k, v in tally.items()})
    np.savez_compressed(args.out, **out)
    print(f"stream seed {gen_seed}: {cols['actions'].numel()} rows in {buffer.size} blocks, tallies {tally}, "
          f"results {results}; wrote {args.out} ({Path(args.out).stat().st_size} bytes)")


if __name__ == "__main__":
    main()
