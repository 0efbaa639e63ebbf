"""Generates tests/golden/g14_selfplay_rollout.npz: the reference's self-play (no-opponent) rollout branch over a synthetic
stream of step results (dev container only: imports the reference tree named by KEISEI_REFERENCE; copies none of its code).

The reference's own ``KataGoRolloutBuffer.add``, ``_compute_value_cats`` and ``fill_alternating_perspective_overrides`` are
driven in the statement order of katago_loop.py:1453-1527 and :1589-1590 over T plies of E envs with a small observation
shape and action space.  The stream is env facts only (movers, rewards, flags, material, the values a model would have
given); games are in progress when it begins, as they are at the start of every epoch but the first.  The fixture holds
the stream, the reference's flattened buffer columns (``next_value_override`` included), ``buffer.size``, the tallies and
the negated bootstrap.

The stream is searched over generator seeds until it reaches every branch (asserted below): a mover's win as black and as
white, a mover's loss, a draw, a truncation without termination, an env done on two consecutive plies, a truncation on
the first and on the last ply, a terminated row directly in front of a non-terminal one of the same env (the pair on
which the alternating fill both skips and acts), and a game decided on the ply that would have truncated it (both flags:
the row takes no override).

    python tools/make_selfplay_golden.py [--out tests/golden/g14_selfplay_rollout.npz]
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
sys.dont_write_bytecode = True

E, T, OBS_SHAPE, A = 4, 24, (2, 3, 3), 40
MAX_PLY = 6
SCORE_NORM = 76.0
KEYS = ("obs", "legal_masks", "pre_players", "actions", "log_probs", "values", "rewards", "terminated", "truncated",
        "current_players", "material", "term_values")


def make_stream(gen_seed: int) -> dict:
    """T plies of env facts: the players alternate inside a game, a game ends by a random result or at MAX_PLY plies, and
    the env starts the next game with player 0 to move.  Every env begins somewhere inside a game."""
    g = np.random.default_rng(gen_seed)
    ply = g.integers(0, MAX_PLY, E)
    player = (ply & 1).astype(np.uint8)
    s = {k: [] for k in KEYS}
    for _ in range(T):
        masks = g.random((E, A)) < 0.3
        actions = g.integers(0, A, E)
        masks[np.arange(E), actions] = True
        ends = g.random(E) < 0.22
        result = g.choice(np.array([1.0, -1.0, 0.0], np.float32), E, p=[0.5, 0.25, 0.25])
        ply = ply + 1
        terminated = ends
        truncated = ply >= MAX_PLY                               # also where the last ply decided the game: both flags
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
    out = {k: np.stack(v) for k, v in s.items()}
    out["final_values"] = (g.random(E) * 2 - 1).astype(np.float32)
    return out


def branches(s: dict) -> set:
    """The branches of the protocol a stream reaches (tests/test_selfplay_rollout_cpu.py asserts the same on the fixture)."""
    tm, tr, r, pre = s["terminated"], s["truncated"], s["rewards"], s["pre_players"]
    done, trunc = tm | tr, tr & ~tm
    seen = set()
    if (tm & (r > 0) & (pre == 0)).any(): seen.add("win_as_black")
    if (tm & (r > 0) & (pre == 1)).any(): seen.add("win_as_white")
    if (tm & (r < 0)).any(): seen.add("loss")
    if (tm & (r == 0)).any(): seen.add("draw")
    if trunc.any(): seen.add("truncation")
    if (done[1:] & done[:-1]).any(): seen.add("done_twice")
    if trunc[0].any(): seen.add("truncation_first_ply")
    if trunc[-1].any(): seen.add("truncation_last_ply")
    if (tm[:-1] & ~done[1:]).any(): seen.add("terminal_before_open")
    if (tm & tr).any(): seen.add("terminated_and_truncated")
    return seen


WANTED = {"win_as_black", "win_as_white", "loss", "draw", "truncation", "done_twice", "truncation_first_ply",
          "truncation_last_ply", "terminal_before_open", "terminated_and_truncated"}


def run_reference(s: dict):
    loop = importlib.import_module("keisei.training.katago_loop")
    ppo = importlib.import_module("keisei.training.katago_ppo")
    dev = torch.device("cpu")
    buffer = ppo.KataGoRolloutBuffer(E, OBS_SHAPE, A)
    tally = dict(wins=0, losses=0, draws=0, black_wins=0, white_wins=0, terminated=0, truncated=0, truncation_overrides=0)
    for t in range(T):
        pre = torch.from_numpy(s["pre_players"][t])
        rewards = torch.from_numpy(s["rewards"][t])
        terminated, truncated = torch.from_numpy(s["terminated"][t]), torch.from_numpy(s["truncated"][t])
        dones = terminated | truncated
        tally["terminated"] += int(terminated.bool().sum())
        tally["truncated"] += int((truncated.bool() & ~terminated.bool()).sum())
        if terminated.any():
            won = rewards[terminated]
            tally["wins"] += int((won > 0).sum()); tally["losses"] += int((won < 0).sum()); tally["draws"] += int((won == 0).sum())
            who = pre[terminated]
            tally["black_wins"] += int((((won > 0) & (who == 0)) | ((won < 0) & (who == 1))).sum())
            tally["white_wins"] += int((((won > 0) & (who == 1)) | ((won < 0) & (who == 0))).sum())
        cats = loop._compute_value_cats(rewards, terminated.bool(), dev)
        score_targets = torch.from_numpy(s["material"][t].astype(np.float32)) / SCORE_NORM
        cut = truncated.bool() & ~terminated.bool()
        override = None
        if bool(cut.any()):
            term_v = torch.from_numpy(s["term_values"][t])
            override = torch.full_like(term_v, float("nan"))
            override[cut] = -term_v[cut]
            tally["truncation_overrides"] += int(cut.sum())
        buffer.add(torch.from_numpy(s["obs"][t]), torch.from_numpy(s["actions"][t]), torch.from_numpy(s["log_probs"][t]),
                   torch.from_numpy(s["values"][t]), rewards, dones, terminated, torch.from_numpy(s["legal_masks"][t]), cats,
                   score_targets, next_value_override=override)
    next_values = -torch.from_numpy(s["final_values"])
    buffer.fill_alternating_perspective_overrides()
    return buffer, tally, next_values


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "g14_selfplay_rollout.npz"))
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
    for gen_seed in range(20000):
        s = make_stream(gen_seed)
        if WANTED <= branches(s):
            break
    else:
        raise SystemExit("no stream seed reaches every branch")
    buffer, tally, next_values = run_reference(s)
    cols = buffer.flatten()
    assert "env_ids" not in cols and "next_value_override" in cols
    ov, tm = cols["next_value_override"].view(T, E), cols["terminated"].view(T, E).bool()
    assert bool(torch.isnan(ov[:-1][tm[:-1]]).all()) and bool(torch.isfinite(ov[:-1][~tm[:-1]]).all())   # the fill skipped and acted
    out = {"stream_" + k: v for k, v in s.items() if k != "final_values"}
    out.update({"col_" + k: v.numpy() for k, v in cols.items()})
    out.update(size=np.int64(buffer.size), gen_seed=np.int64(gen_seed), score_norm=np.float64(SCORE_NORM),
               obs_shape=np.array(OBS_SHAPE, np.int64), action_space=np.int64(A), final_values=s["final_values"],
               next_values=next_values.numpy(), **{"tally_" + k: np.int64(v) for k, v in tally.items()})
    np.savez_compressed(args.out, **out)
    print(f"stream seed {gen_seed}: {cols['actions'].numel()} rows in {buffer.size} steps, tallies {tally}; "
          f"wrote {args.out} ({Path(args.out).stat().st_size} bytes)")


if __name__ == "__main__":
    main()
