"""Generates tests/golden/g12_game_features.npz: the reference's GameFeatureTracker rows for two step streams (dev container
only: imports the reference module named by KEISEI_REFERENCE unchanged; copies none of its code).

  (a) a CPU-oracle playout: OracleVecEnv(64, max_ply=60), 400 plies of seeded uniform legal play, pre_step_players = the
      previous step's current_players (zeros after reset);
  (b) a synthetic stream (``synthetic_stream`` below, which the tests import too) for what random play does not reach:
      termination reasons 0..5 on finished steps, rewards -1 / 0 / +1 / NaN for both movers, game lengths across the 20 / 30 /
      40 ply windows, source squares 76 and 79, move types at the edges of the promotion and drop ranges (63/64, 131/132,
      138), reason 2 on steps that do not finish a game, and one env whose ply count crosses 32767 (a uint16 payload).

The fixture holds per stream the step arrays (T, N) in their narrow dtypes and the rows as columns (``pack_rows`` /
``unpack_rows``), and ``classify`` = classify_action over all 11 259 actions (bit 0 drop, bit 1 promotion) with
``classify_square``.  Every integer column must take at least two values and every optional column must be both None and
set, over the two streams together; the generator asserts it.

    python tools/make_features_golden.py [--out tests/golden/g12_game_features.npz]
"""
from __future__ import annotations

import argparse
import importlib.util
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
REF = Path(os.environ.get("KEISEI_REFERENCE") or ROOT.parent / "reference")
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
sys.dont_write_bytecode = True

A = 81 * 139
STEP_KEYS = ("actions", "captured_piece", "termination_reason", "ply_count", "pre_players", "terminated", "truncated", "rewards")
STEP_DTYPES = dict(actions=np.int16, captured_piece=np.uint8, termination_reason=np.uint8, ply_count=np.uint16,
                   pre_players=np.uint8, terminated=np.bool_, truncated=np.bool_, rewards=np.float32)
ROW_KEYS = ("checkpoint_id", "opponent_id", "epoch", "side", "result", "total_plies", "first_action", "opening_seq_3",
            "opening_seq_6", "rook_moved_ply", "king_displacement_20", "first_capture_ply", "first_drop_ply", "num_captures",
            "num_drops", "num_promotions", "num_early_drops", "rook_moves_in_20", "king_moves_in_30", "num_repetitions",
            "termination_reason")
STRING_KEYS = ("side", "result", "opening_seq_3", "opening_seq_6")
OPTIONAL_KEYS = ("first_action", "opening_seq_3", "opening_seq_6", "rook_moved_ply", "first_capture_ply", "first_drop_ply")
SYNTH = dict(num_envs=24, plies=240, seed=12)                # stream (b) of the fixture
IDS = {"a": (7, 3, 2), "b": (11, 5, 9)}                      # entry_a_id, entry_b_id, epoch per stream


def synthetic_stream(num_envs: int, plies: int, seed: int, p_done: float = 0.05) -> list:
    """Per ply a dict of the eight ``record_step`` arrays over ``num_envs`` envs (STEP_KEYS, STEP_DTYPES; actions int64).
    Each env counts its game's plies and alternates its mover from player 0; env 0's count starts at 32 766."""
    rng = np.random.default_rng(seed)
    count = np.zeros(num_envs, np.int64)
    offset = np.zeros(num_envs, np.int64)
    offset[0] = 32766
    squares = np.array([76, 79])
    types = np.array([63, 64, 131, 132, 138, 0, 127, 128])
    out = []
    for _ in range(plies):
        count += 1
        sq = np.where(rng.random(num_envs) < 0.35, rng.choice(squares, num_envs), rng.integers(0, 81, num_envs))
        mt = np.where(rng.random(num_envs) < 0.5, rng.choice(types, num_envs), rng.integers(0, 139, num_envs))
        done = rng.random(num_envs) < p_done
        both = rng.random(num_envs) < 0.1
        term = done & ((rng.random(num_envs) < 0.6) | both)
        trunc = done & (~term | both)
        reason = np.where(done, rng.integers(0, 6, num_envs), np.where(rng.random(num_envs) < 0.1, 2, 0))
        rewards = np.where(done, rng.choice(np.array([-1.0, 0.0, 1.0, np.nan]), num_envs, p=[0.35, 0.2, 0.35, 0.1]),
                           np.where(rng.random(num_envs) < 0.05, 1.0, 0.0))
        captured = np.where(rng.random(num_envs) < 0.25, rng.integers(0, 7, num_envs), 255)
        out.append(dict(actions=(sq * 139 + mt).astype(np.int64), captured_piece=captured.astype(np.uint8),
                        termination_reason=reason.astype(np.uint8), ply_count=(count + offset).astype(np.uint16),
                        pre_players=((count - 1) & 1).astype(np.uint8), terminated=term, truncated=trunc,
                        rewards=rewards.astype(np.float32)))
        count[done], offset[done] = 0, 0
    return out


def oracle_stream(num_envs: int = 64, max_ply: int = 60, plies: int = 400, seed: int = 5) -> list:
    from oracle.shogi import OracleVecEnv

    env = OracleVecEnv(num_envs, max_ply)
    _, mask = env.reset()
    rng = np.random.default_rng(seed)
    pre = np.zeros(num_envs, np.uint8)
    out = []
    for _ in range(plies):
        actions = np.array([rng.choice(np.flatnonzero(m)) for m in mask], dtype=np.int64)
        r = env.step(actions)
        out.append(dict(actions=actions, captured_piece=r["captured_piece"], termination_reason=r["termination_reason"],
                        ply_count=r["ply_count"], pre_players=pre, terminated=r["terminated"], truncated=r["truncated"],
                        rewards=r["rewards"]))
        pre, mask = r["current_players"].copy(), r["legal_masks"]
    return out


def run_tracker(tracker, stream) -> list:
    for p in stream:
        tracker.record_step(*(p[k] for k in STEP_KEYS))
    return [r.to_dict() for r in tracker.completed_rows]


def pack_rows(rows: list, prefix: str) -> dict:
    out = {}
    for k in ROW_KEYS:
        none = np.array([r[k] is None for r in rows])
        if k in STRING_KEYS:
            out[prefix + k] = np.array([(r[k] or "").encode() for r in rows], dtype=np.bytes_)
        else:
            out[prefix + k] = np.array([0 if r[k] is None else r[k] for r in rows], dtype=np.int32)
        if k in OPTIONAL_KEYS:
            out[prefix + k + ".none"] = none
        else:
            assert not none.any(), k
    return out


def unpack_rows(z, prefix: str) -> list:
    cols = {}
    for k in ROW_KEYS:
        v = z[prefix + k]
        vals = [x.decode() for x in v] if k in STRING_KEYS else [int(x) for x in v]
        if k in OPTIONAL_KEYS:
            vals = [None if n else x for x, n in zip(vals, z[prefix + k + ".none"])]
        cols[k] = vals
    return [{k: cols[k][i] for k in ROW_KEYS} for i in range(len(cols["side"]))]


def stream_arrays(z, prefix: str) -> list:
    """The fixture's step arrays of one stream back as the per-ply dicts ``run_tracker`` takes."""
    cols = {k: z[prefix + k] for k in STEP_KEYS}
    return [{k: cols[k][t] for k in STEP_KEYS} for t in range(cols["actions"].shape[0])]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "g12_game_features.npz"))
    args = ap.parse_args()
    src = REF / "keisei" / "training" / "game_feature_tracker.py"
    if not src.is_file():
        sys.exit(f"needs the reference tree at {REF} (dev container only)")
    spec = importlib.util.spec_from_file_location("_reference_game_feature_tracker", src)
    ref = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = ref                             # dataclasses look their module up by name
    spec.loader.exec_module(ref)

    out, all_rows = {}, []
    for name, stream in (("a", oracle_stream()), ("b", synthetic_stream(**SYNTH))):
        ida, idb, epoch = IDS[name]
        rows = run_tracker(ref.GameFeatureTracker(len(stream[0]["actions"]), ida, idb, epoch), stream)
        assert [list(r) for r in rows[:1]] == [list(ROW_KEYS)], "the reference's columns changed"
        for k in STEP_KEYS:
            col = np.stack([p[k] for p in stream])
            assert np.array_equal(col.astype(STEP_DTYPES[k]).astype(col.dtype), col, equal_nan=k == "rewards"), k
            out[f"{name}.{k}"] = col.astype(STEP_DTYPES[k])
        out.update(pack_rows(rows, f"{name}.rows."))
        out[f"{name}.ids"] = np.array([ida, idb, epoch], np.int64)
        reasons = sorted({r["termination_reason"] for r in rows})
        print(f"stream ({name}): {len(stream)} plies x {len(stream[0]['actions'])} envs, {len(rows)} rows, reasons {reasons}, "
              + ", ".join(f"{k} None {sum(r[k] is None for r in rows)}" for k in OPTIONAL_KEYS))
        all_rows += rows
    for k in ROW_KEYS:
        values = {r[k] for r in all_rows}
        assert len(values - {None}) >= 2, f"column {k} takes one value only"
        if k in OPTIONAL_KEYS:
            assert None in values and len(values) > 1, f"optional column {k} is not both None and set"
    synth = [r for r in all_rows if r["checkpoint_id"] in IDS["b"][:2]]
    assert {r["termination_reason"] for r in synth} == set(range(6))
    assert {(r["side"], r["result"]) for r in synth} == {(s, x) for s in ("black", "white") for x in ("win", "loss", "draw")}
    assert max(r["total_plies"] for r in synth) > 32767

    table = [ref.classify_action(a) for a in range(A)]
    out["classify"] = np.array([int(d) | int(p) << 1 for d, p, _ in table], np.uint8)
    out["classify_square"] = np.array([s for _, _, s in table], np.uint8)
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out} ({Path(args.out).stat().st_size} bytes)")


if __name__ == "__main__":
    main()
