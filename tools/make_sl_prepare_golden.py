"""Generates tests/golden/g15_sl_prepare.npz, g15_games.sfen and g15_games.csa: game records for keisei_amd.sl.prepare and
what a replay of them has to give (dev container only: imports the reference tree named by KEISEI_REFERENCE for its
parsers and the CPU env oracle; copies none of the reference's code).

Game text comes from seeded playouts of ``OracleVecEnv`` (random legal moves, leaning towards captures, promotions and
drops so that short games have them), decoded to USI for the .sfen file and to CSA moves for the .csa file:

  - plain games of 1 to 60 moves, outcomes black / white / draw, both files;
  - a game that ends in checkmate (a mate in one is played when there is one; found by seed search) with two junk moves
    behind the mate;
  - an illegal (but encodable) move at ply 0, in the middle, as the last move;
  - a move the spatial planes cannot hold;
  - a game longer than MAX_MOVES;
  - a game from a handicap position, games without a known result.

The fixture holds (a) the REFERENCE parsers' output on the two files -- moves, outcomes, metadata -- as string arrays,
(b) per game the number of positions a replay keeps and why it stops there, (c) per kept position the policy index
(``oracle.shogi.encode``), the W/D/L category by the reference's rule (prepare.py:137-149), the material balance after the
move and a 64-bit checksum of the observation before it.  (b) and (c) come from a plain one-game-at-a-time replay
written here, not from the package.

    python tools/make_sl_prepare_golden.py [--out-dir tests/golden]
"""
from __future__ import annotations

import argparse
import os
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
REF = Path(os.environ.get("KEISEI_REFERENCE", "/root/reference"))
sys.dont_write_bytecode = True
sys.path.insert(0, str(ROOT))

from oracle import shogi as so  # noqa: E402

MAX_MOVES = 96                   # the replay's cap in the fixture (the "long" game has more)
A = so.A_SIZE
RANKS = "abcdefghi"
HAND = "?PLNSGBR"
CSA_NAME = {1: "FU", 2: "KY", 3: "KE", 4: "GI", 5: "KI", 6: "KA", 7: "HI", 8: "OU"}
CSA_PROMOTED = {1: "TO", 2: "NY", 3: "NK", 4: "NG", 6: "UM", 7: "RY"}
REASONS = ("none", "illegal move", "ended by the rules", "longer than max_moves", "no spatial encoding")
HANDICAP_SFEN = "lnsgkgsnl/1r5b1/ppppppppp/9/9/9/PPPPPPPPP/7R1/LNSGKGSNL w - 1"
CSA_BOARD = """P1-KY-KE-GI-KI-OU-KI-GI-KE-KY
P2 * -HI *  *  *  *  * -KA *
P3-FU-FU-FU-FU-FU-FU-FU-FU-FU
P4 *  *  *  *  *  *  *  *  *
P5 *  *  *  *  *  *  *  *  *
P6 *  *  *  *  *  *  *  *  *
P7+FU+FU+FU+FU+FU+FU+FU+FU+FU
P8 * +KA *  *  *  *  * +HI *
P9+KY+KE+GI+KI+OU+KI+GI+KE+KY"""


def obs_checksum(obs: np.ndarray) -> np.uint64:
    """64-bit position-weighted sum of the observation's bit patterns (wraps modulo 2^64)."""
    w = np.ascontiguousarray(obs, dtype=np.float32).reshape(-1).view(np.uint32).astype(np.uint64)
    k = np.arange(w.size, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(0xD1B54A32D192ED03)
    with np.errstate(over="ignore"):
        return np.uint64((w * k).sum(dtype=np.uint64))


def sq_usi(sq: int) -> str:
    return f"{9 - sq % 9}{RANKS[sq // 9]}"


def sq_csa(sq: int) -> str:
    return f"{9 - sq % 9}{sq // 9 + 1}"


def move_text(idx: int, white: bool, board: np.ndarray):
    """(USI, CSA) text of action ``idx`` in a position with ``board`` (piece bytes: type | 0x10 white | 0x20 promoted)."""
    frm, to, promote, drop = so.decode(idx, white)
    sign = "-" if white else "+"
    if drop:
        return f"{HAND[drop]}*{sq_usi(to)}", f"{sign}00{sq_csa(to)}{CSA_NAME[drop]}"
    piece = int(board[frm])
    kind, promoted = piece & 15, bool(piece & so.PROM) or bool(promote)
    name = CSA_PROMOTED[kind] if promoted and kind in CSA_PROMOTED else CSA_NAME.get(kind, "FU")
    return f"{sq_usi(frm)}{sq_usi(to)}" + ("+" if promote else ""), f"{sign}{sq_csa(frm)}{sq_csa(to)}{name}"


def playout(seed: int, length: int, *, mate: bool = False, max_ply: int = 400):
    """A seeded playout: list of (USI, CSA, kinds) per move, and how it ended (termination reason or None)."""
    rng = np.random.default_rng(seed)
    env, probe = so.OracleVecEnv(1, max_ply), so.OracleVecEnv(1, max_ply)
    _, mask = env.reset()
    moves, white = [], False
    for _ in range(length):
        legal = np.nonzero(mask[0])[0]
        board, hands, side, _ply = env.state(0)
        choice = None
        if mate:                                                # play a mate in one when there is one
            for a in legal:
                probe.set_state(0, board, hands, side)
                r = probe.step([int(a)])
                if r["terminated"][0] and r["termination_reason"][0] == so.R_CHECKMATE:
                    choice = int(a)
                    break
        if choice is None:
            dec = [so.decode(int(a), white) for a in legal]
            lively = [int(a) for a, (f, t, p, d) in zip(legal, dec) if d or p or board[t]]
            choice = int(rng.choice(lively)) if lively and rng.random() < 0.6 else int(rng.choice(legal))
        f, t, p, d = so.decode(choice, white)
        kinds = ("drop" if d else "promote" if p else "capture" if board[t] else "quiet") + ("_w" if white else "_b")
        moves.append((*move_text(choice, white, board), kinds))
        r = env.step([choice])
        if r["terminated"][0] or r["truncated"][0]:
            return moves, int(r["termination_reason"][0])
        mask, white = r["legal_masks"], not white
    return moves, None


def parse_usi(usi: str):
    """(from, to, promote, drop) of well-formed USI text, None otherwise.  Written for this tool: the fixture must not
    depend on the package's own conversion."""
    if len(usi) == 4 and usi[1] == "*" and usi[0] in HAND[1:] and usi[2] in "123456789" and usi[3] in RANKS:
        return 0, RANKS.index(usi[3]) * 9 + 9 - int(usi[2]), 0, HAND.index(usi[0])
    if len(usi) in (4, 5) and usi[0] in "123456789" and usi[1] in RANKS and usi[2] in "123456789" and usi[3] in RANKS \
            and (len(usi) == 4 or usi[4] == "+"):
        return RANKS.index(usi[1]) * 9 + 9 - int(usi[0]), RANKS.index(usi[3]) * 9 + 9 - int(usi[2]), int(len(usi) == 5), 0
    return None


def encodable(frm, to, promote, drop, white) -> int:
    """oracle.shogi.encode, -1 where the spatial planes cannot hold the move (the index must decode to the same move)."""
    if not drop and frm == to:
        return -1
    idx = so.encode(frm, to, bool(promote), drop, white)
    if idx < 0 or idx >= A:
        return -1
    back = so.decode(idx, white)
    if back is None or (not drop and tuple(back) != (frm, to, promote, 0)) or (drop and (back[1], back[3]) != (to, drop)):
        return -1
    return idx


def replay_one(moves, outcome: str):
    """One game, one env: the kept positions and why the replay stops.  The reference's value rule (prepare.py:137-149)."""
    env = so.OracleVecEnv(1, MAX_MOVES)
    obs, mask = env.reset()
    pos, reason = [], 0
    for i, usi in enumerate(moves):
        if i >= MAX_MOVES:
            reason = 3
            break
        mv = parse_usi(usi)
        idx = encodable(*mv, bool(i & 1)) if mv is not None else -1
        if idx < 0:
            reason = 4
            break
        if not mask[0, idx]:
            reason = 1
            break
        black_to_move = i % 2 == 0
        value = 1 if outcome == "draw" else (0 if (outcome == "win_black") == black_to_move else 2)
        r = env.step([idx])
        pos.append((idx, value, int(r["material_balance"][0]), obs_checksum(obs[0])))
        if (r["terminated"][0] or r["truncated"][0]) and i + 1 < min(len(moves), MAX_MOVES):
            reason = 2
            break
        obs, mask = r["observations"], r["legal_masks"]
    return pos, reason


def some_illegal(prefix, rng):
    """(USI, CSA) of an encodable move that is NOT legal after the USI moves ``prefix``."""
    env = so.OracleVecEnv(1, 400)
    _, mask = env.reset()
    for i, usi in enumerate(prefix):
        mask = env.step([encodable(*parse_usi(usi), bool(i & 1))])["legal_masks"]
    white = bool(len(prefix) & 1)
    board = env.state(0)[0]
    for idx in rng.permutation(A):
        d = so.decode(int(idx), white)
        if mask[0, idx] or d is None or d[2] or (not d[3] and d[0] == d[1]):
            continue
        if encodable(*d, white) != int(idx):
            continue
        return move_text(int(idx), white, board)
    raise RuntimeError("no illegal move found")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out-dir", default=str(ROOT / "tests" / "golden"))
    out_dir = Path(ap.parse_args().out_dir)
    rng = np.random.default_rng(15)

    # ------------------------------------------------------------------ the games
    games = []                                                  # dicts: tag, fmt, result, moves [(usi, csa)], meta, start

    def add(tag, fmt, result, moves, start="startpos", **meta):
        if fmt == "csa" and result.startswith("win"):           # a CSA game ends in %TORYO here: the last mover wins
            result = "win_black" if len(moves) % 2 == 1 else "win_white"
        # (the CSA sign follows the ply: spliced-in moves come from other positions)
        moves = [(m[0], "+-"[k & 1] + m[1][1:]) for k, m in enumerate(moves)]
        games.append(dict(tag=tag, fmt=fmt, result=result, moves=moves, start=start, meta=meta))

    lengths = [1, 7, 12, 18, 23, 29, 34, 40, 45, 51, 56, 60]
    results = ["win_black", "win_white", "draw"]
    kinds = set()
    for k, n in enumerate(lengths):
        seed = 1000 + k
        while True:
            moves, ended = playout(seed, n)
            if ended is None and len(moves) == n:
                break
            seed += 100
        kinds.update(m[2] for m in moves)
        add(f"plain{n}", "sfen" if k % 2 == 0 else "csa", results[k % 3], moves, black_rating=str(1500 + 40 * k),
            white_rating=str(1400 + 35 * k))
    need = {f"{a}_{c}" for a in ("drop", "promote", "capture") for c in "bw"}
    assert need <= kinds, need - kinds

    seed = 0
    while True:                                                 # a checkmate that leaves room under MAX_MOVES
        moves, ended = playout(seed, MAX_MOVES - 8, mate=True)
        if ended == so.R_CHECKMATE and len(moves) >= 10:
            break
        seed += 1
    mate_len, mate_seed = len(moves), seed
    winner = "win_black" if mate_len % 2 == 1 else "win_white"
    junk, _ = playout(7, 2)
    add("mate_sfen", "sfen", winner, moves + junk)
    add("mate_csa", "csa", winner, moves + junk)

    base, _ = playout(2001, 24)
    add("illegal_first", "sfen", "win_white", [some_illegal([], rng)] + base[:10])
    add("illegal_middle", "csa", "win_black", base[:11] + [some_illegal([m[0] for m in base[:11]], rng)] + base[12:24])
    add("illegal_last", "sfen", "draw", base[:16] + [some_illegal([m[0] for m in base[:16]], rng)])
    assert encodable(*parse_usi("5i3f"), False) < 0 and encodable(*parse_usi("8b5a"), True) < 0
    add("no_encoding_sfen", "sfen", "win_black", base[:6] + [("5i3f", "+5936OU")] + base[7:12])
    add("no_encoding_csa", "csa", "win_white", base[:9] + [("8b5a", "-8251HI")] + base[10:14])
    seed = 3000
    while True:
        long_moves, ended = playout(seed, MAX_MOVES + 14)
        if ended is None:
            break
        seed += 1
    add("long_sfen", "sfen", "win_black", long_moves)
    add("long_csa", "csa", "draw", long_moves[:MAX_MOVES + 5])
    add("handicap", "sfen", "win_white", base[:8], start=HANDICAP_SFEN)
    add("no_result_sfen", "sfen", "aborted", base[:9])
    add("no_result_csa", "csa", "%CHUDAN", base[:9])
    add("pi_start", "csa", "win_black", base[:13], start="PI")
    add("handicap_csa", "csa", "win_white", base[:5], start="PI82HI22KA")

    # ------------------------------------------------------------------ the files
    sfen_blocks, csa_blocks = [], []
    for g in games:
        if g["fmt"] == "sfen":
            head = [f"result:{g['result']}"] + [f"{k}:{v}" for k, v in g["meta"].items()]
            sfen_blocks.append("\n".join(head + [g["start"]] + [m[0] for m in g["moves"]]))
        else:
            end = {"draw": "%SENNICHITE", "%CHUDAN": "%CHUDAN"}.get(g["result"], "%TORYO")
            head = ["V2.2", f"N+{g['tag']}_sente", f"N-{g['tag']}_gote", "$EVENT:g15"]
            head += [f"${k.upper()}:{v}" for k, v in g["meta"].items()]
            head += [CSA_BOARD] if g["start"] == "startpos" else [g["start"]]
            body = []
            for m in g["moves"]:
                body += [m[1], "T1"]
            csa_blocks.append("\n".join(head + ["+"] + body + [end]))
    out_dir.mkdir(parents=True, exist_ok=True)
    (out_dir / "g15_games.sfen").write_text("\n\n".join(sfen_blocks) + "\n")
    (out_dir / "g15_games.csa").write_text("\n/\n".join(csa_blocks) + "\n")

    # ------------------------------------------------------------------ the reference's parsers on them
    sys.path.insert(0, str(REF))
    from keisei.sl.parsers import CSAParser, SFENParser
    records, file_of = [], []
    for k, (parser, name) in enumerate(((SFENParser(), "g15_games.sfen"), (CSAParser(), "g15_games.csa"))):
        recs = list(parser.parse(out_dir / name))
        records += recs
        file_of += [k] * len(recs)
    parsed_tags = [g["tag"] for g in games if g["fmt"] == "sfen" and g["result"] != "aborted"] + \
                  [g["tag"] for g in games if g["fmt"] == "csa" and g["result"] != "%CHUDAN"]
    assert len(records) == len(parsed_tags), (len(records), len(parsed_tags))
    by_tag = {g["tag"]: g for g in games}
    for rec, tag in zip(records, parsed_tags):                  # the CSA text says what the USI text says
        assert [m.move_usi for m in rec.moves] == [m[0] for m in by_tag[tag]["moves"]], tag
        assert rec.outcome.value == by_tag[tag]["result"], tag
    standard = np.array([by_tag[t]["start"] in ("startpos", "PI") for t in parsed_tags])

    # ------------------------------------------------------------------ the replay
    valid_len, reason, pol, val, mat, chk, game_of = [], [], [], [], [], [], []
    for g, (rec, ok) in enumerate(zip(records, standard)):
        if not ok:
            valid_len.append(0)
            reason.append(0)
            continue
        pos, why = replay_one([m.move_usi for m in rec.moves], rec.outcome.value)
        valid_len.append(len(pos))
        reason.append(why)
        for p in pos:
            pol.append(p[0]); val.append(p[1]); mat.append(p[2]); chk.append(p[3]); game_of.append(g)
    reason_a = np.array(reason)
    expect = {"illegal_first": (0, 1), "illegal_middle": (11, 1), "illegal_last": (16, 1), "no_encoding_sfen": (6, 4),
              "no_encoding_csa": (9, 4), "long_sfen": (MAX_MOVES, 3), "long_csa": (MAX_MOVES, 3),
              "mate_sfen": (mate_len, 2), "mate_csa": (mate_len, 2), "plain1": (1, 0), "pi_start": (13, 0)}
    for tag, want in expect.items():
        g = parsed_tags.index(tag)
        assert (valid_len[g], reason[g]) == want, (tag, valid_len[g], reason[g], want)
    meta_keys, meta_vals, meta_game = [], [], []
    for g, rec in enumerate(records):
        for k, v in rec.metadata.items():
            meta_keys.append(k); meta_vals.append(v); meta_game.append(g)
    lens = np.array([len(r.moves) for r in records])
    np.savez_compressed(
        out_dir / "g15_sl_prepare.npz",
        max_moves=np.int64(MAX_MOVES), tags=np.array(parsed_tags), file_of=np.array(file_of, np.int64),
        moves=np.array([m.move_usi for r in records for m in r.moves]), move_offsets=np.concatenate(([0], np.cumsum(lens))),
        outcomes=np.array([r.outcome.value for r in records]), meta_keys=np.array(meta_keys), meta_vals=np.array(meta_vals),
        meta_game=np.array(meta_game, np.int64), standard_start=standard,
        valid_len=np.array(valid_len, np.int64), reason=reason_a.astype(np.int64), reason_names=np.array(REASONS),
        pos_game=np.array(game_of, np.int64), pos_policy=np.array(pol, np.int64), pos_value=np.array(val, np.int64),
        pos_material=np.array(mat, np.int64), pos_checksum=np.array(chk, np.uint64),
        games_cut_illegal=np.int64(((reason_a == 1) | (reason_a == 4)).sum()), games_cut_by_rules=np.int64((reason_a == 2).sum()),
        games_cut_long=np.int64((lens[standard] > MAX_MOVES).sum()), games_nonstandard_start=np.int64((~standard).sum()),
        mate_len=np.int64(mate_len))
    print(f"{len(records)} parsed games ({len(games)} written), {len(pol)} positions, mate in {mate_len} (seed {mate_seed}); "
          f"reasons {dict(zip(*np.unique(reason_a, return_counts=True)))}")
    for name in ("g15_sl_prepare.npz", "g15_games.sfen", "g15_games.csa"):
        print(f"  {name}: {(out_dir / name).stat().st_size} bytes")


if __name__ == "__main__":
    main()
