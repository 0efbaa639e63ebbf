"""Device-resident mirror of the reference's `shogi_gym.VecEnv`.

Reference: shogi-engine/crates/shogi-gym/src/vec_env.rs:556-855 (the PyO3 class), step_result.rs:31-97 (result types).
Same constructor, `reset()` / `step(actions)`, result attributes, counters and error behaviour -- but the N games live in
HBM and a step is two launches of `shogi_env.hip` (C ABI `ka_shogi_env_*`, include/keisei_amd.h).  Both observation modes
("default" 46 planes, "katago" 50) and both action modes ("default" 13 527 actions, "spatial" 11 259) exist; the KataGo loop
asks for katago + spatial (katago_loop.py:580-585).  `DefaultActionMapper` / `SpatialActionMapper` are the index arithmetic of
action_mapper.rs / spatial_action_mapper.rs on the host.

`output="numpy"` (default) returns host arrays like the reference does; `output="torch"` returns the device tensors
themselves -- every per-step field of a result (observations, masks, rewards, flags, players, metadata) alternates
between two buffers, so a StepResult stays intact until the step after the next one; keep `.clone()`s of what must live
longer.  `terminal_observations` is the reference's ONE persistent buffer (vec_env.rs:246): the row of a game that ended
stays until that game ends again.  This is the form `select_actions` and the device rollout store consume without a host round trip.
A refused step (an illegal action anywhere) moves nothing: the kernel then writes the unchanged positions' observations
and masks (zero rewards, no flags) into the buffers the caller flips to, so a caller that runs with `check_actions=False`
and reads the flag late (`raise_if_refused()`) has still stepped against the right masks.
`VecEnv(..., start_pool_capacity=K)` (not in the reference) keeps a pool of up to K start positions in device memory:
after `set_start_positions` / `set_start_sfens` the games of `reset()` and every game the kernel restarts begin at a pool
row drawn per (seed, env, game number) -- `start_pool_index` is the same draw on the host -- instead of the standard
position; `clear_start_positions()` returns to it.  Uploads are validated here, because the kernel assumes playable
positions.  `parse_sfen` / `format_sfen` are the text form of a position.
`get_spectator_data()` returns the reference's spectator dicts from one read of the state rows; `VecEnv(...,
move_history=True)` (keyword-only) makes `step()` keep one note per move of each game in progress (csrc/spectator.hip, two
more launches; cleared when the game ends, unchanged by a refused step), from which `hodges_notation` / `move_usi` give
the reference's `move_history` entries.
There is no CPU fallback: without the HIP library or a GPU the constructor raises.
"""
from __future__ import annotations

import weakref
from dataclasses import dataclass
from typing import Any, List, Optional

import numpy as np
import torch

from . import _lib

ACTION_SPACE = 81 * 139            # spatial
DEFAULT_ACTION_SPACE = 81 * 80 * 2 + 81 * 7
OBS_CHANNELS = 50                  # katago
DEFAULT_OBS_CHANNELS = 46
MASK_WORDS = (ACTION_SPACE + 31) // 32
_DIRS = ((-1, 0), (-1, 1), (0, 1), (1, 1), (1, 0), (1, -1), (0, -1), (-1, -1))     # spatial_action_mapper.rs:31-40


def _sq(v: int, what: str) -> int:
    if not 0 <= v < 81:
        raise ValueError(f"invalid square index: {v}")
    return v


class SpatialActionMapper:
    """spatial_action_mapper.rs:138-356: flat index = square * 139 + move type, in the mover's perspective."""

    action_space_size = ACTION_SPACE

    def encode_board_move(self, from_sq: int, to_sq: int, promote: bool, is_white: bool) -> int:
        f, t = _sq(from_sq, "from"), _sq(to_sq, "to")
        if f == t:
            raise ValueError("from_sq and to_sq must be different")
        if is_white:
            f, t = 80 - f, 80 - t
        dr, dc = t // 9 - f // 9, t % 9 - f % 9
        if dr == 0 or dc == 0 or abs(dr) == abs(dc):
            unit = ((dr > 0) - (dr < 0), (dc > 0) - (dc < 0))
            return f * 139 + (64 if promote else 0) + _DIRS.index(unit) * 8 + max(abs(dr), abs(dc)) - 1
        if abs(dr) == 2 and abs(dc) == 1:
            same = (dr > 0) == (dc > 0)
            return f * 139 + 128 + (0 if same else 1) * 2 + (1 if promote else 0)
        raise ValueError(f"Cannot encode board move from ({f // 9},{f % 9}) to ({t // 9},{t % 9}) — not a valid direction, "
                         "distance, or knight move")

    def encode_drop_move(self, to_sq: int, piece_type_idx: int, is_white: bool) -> int:
        t = _sq(to_sq, "to")
        if not 0 <= piece_type_idx < 7:
            raise ValueError(f"piece_type_idx {piece_type_idx} out of range (max 6)")
        return (80 - t if is_white else t) * 139 + 132 + piece_type_idx

    def decode(self, idx: int, is_white: bool) -> dict:
        if not 0 <= idx < ACTION_SPACE:
            raise ValueError(f"action index {idx} out of range (max {ACTION_SPACE - 1})")
        s, slot = divmod(idx, 139)
        flip = (lambda q: 80 - q) if is_white else (lambda q: q)
        if slot >= 132:
            return {"type": "drop", "to_sq": flip(s), "piece_type_idx": slot - 132}
        if slot < 128:
            promote, b = slot >= 64, slot & 63
            dr, dc = _DIRS[b // 8]
            r, c = s // 9 + dr * (b % 8 + 1), s % 9 + dc * (b % 8 + 1)
        else:
            promote, (r, c) = bool((slot - 128) & 1), (s // 9 - 2, s % 9 + (-1 if (slot - 128) // 2 == 0 else 1))
        if not (0 <= r < 9 and 0 <= c < 9):
            raise ValueError(f"decoded move goes off board: from ({s // 9},{s % 9}) slot={slot}")
        return {"type": "board", "from_sq": flip(s), "to_sq": flip(r * 9 + c), "promote": promote}


class DefaultActionMapper:
    """action_mapper.rs:17-222: from * 160 + (to skipping from) * 2 + promote, then 81 x 7 drops."""

    action_space_size = DEFAULT_ACTION_SPACE

    def encode_board_move(self, from_sq: int, to_sq: int, promote: bool, is_white: bool) -> int:
        f, t = _sq(from_sq, "from"), _sq(to_sq, "to")
        if f == t:
            raise ValueError("from_sq and to_sq must be different")
        if is_white:
            f, t = 80 - f, 80 - t
        return f * 160 + (t - 1 if t > f else t) * 2 + (1 if promote else 0)

    def encode_drop_move(self, to_sq: int, piece_type_idx: int, is_white: bool) -> int:
        t = _sq(to_sq, "to")
        if not 0 <= piece_type_idx < 7:
            raise ValueError(f"piece_type_idx {piece_type_idx} is out of range (max 6)")
        return 81 * 160 + (80 - t if is_white else t) * 7 + piece_type_idx

    def decode(self, idx: int, is_white: bool) -> dict:
        if not 0 <= idx < DEFAULT_ACTION_SPACE:
            raise ValueError(f"action index {idx} is out of range (max {DEFAULT_ACTION_SPACE - 1})")
        flip = (lambda q: 80 - q) if is_white else (lambda q: q)
        if idx >= 81 * 160:
            t, h = divmod(idx - 81 * 160, 7)
            return {"type": "drop", "to_sq": flip(t), "piece_type_idx": h}
        f, rem = divmod(idx, 160)
        off = rem // 2
        return {"type": "board", "from_sq": flip(f), "to_sq": flip(off + 1 if off >= f else off), "promote": bool(rem & 1)}

_SFEN = {1: "P", 2: "L", 3: "N", 4: "S", 5: "G", 6: "B", 7: "R", 8: "K"}
_SFEN_TYPE = {v: k for k, v in _SFEN.items()}
_PROMOTABLE = (1, 2, 3, 4, 6, 7)
_SET_MAX = (18, 4, 4, 4, 4, 2, 2)                             # P L N S G B R of a standard set, board and hands together
POOL_ROW_BYTES = 96                                           # a start-pool row: board[81] hands[14] side


def format_sfen(board, hands, side: int) -> str:
    """sfen.rs:93-171: board rows from rank a, side to move, hands (R B G S N L P, black first), move number 1."""
    board = np.asarray(board, np.uint8).reshape(81)
    hands = np.asarray(hands, np.uint8).reshape(2, 7)
    rows = []
    for r in range(9):
        s, empty = "", 0
        for c in range(9):
            p = int(board[r * 9 + c])
            if not p:
                empty += 1
                continue
            if empty:
                s, empty = s + str(empty), 0
            ch = _SFEN[p & 15]
            s += ("+" if p & 0x20 else "") + (ch.lower() if p & 0x10 else ch)
        rows.append(s + (str(empty) if empty else ""))
    hs = ""
    for color in (0, 1):
        for h in (6, 5, 4, 3, 2, 1, 0):                       # R B G S N L P
            cnt = int(hands[color, h])
            if cnt:
                ch = _SFEN[h + 1]
                hs += (str(cnt) if cnt > 1 else "") + (ch.lower() if color else ch)
    return f"{'/'.join(rows)} {'w' if side else 'b'} {hs or '-'} 1"


def parse_sfen(sfen: str):
    """The inverse of `format_sfen` (sfen.rs:17-91): `(board uint8[81], hands uint8[2, 7], side)`; the move number is
    optional and ignored.  A malformed string raises `ValueError` naming the string and the field."""
    def bad(field: str, why: str):
        return ValueError(f"invalid SFEN {sfen!r}: {field} field: {why}")

    if not isinstance(sfen, str):
        raise ValueError(f"invalid SFEN {sfen!r}: not a string")
    parts = sfen.split()
    if len(parts) not in (3, 4):
        raise ValueError(f"invalid SFEN {sfen!r}: expected 'board side hands [move number]', got {len(parts)} fields")
    board, hands = np.zeros(81, np.uint8), np.zeros((2, 7), np.uint8)
    rows = parts[0].split("/")
    if len(rows) != 9:
        raise bad("board", f"{len(rows)} ranks, expected 9")
    for r, row in enumerate(rows):
        c, prom = 0, False
        for ch in row:
            if ch == "+":
                if prom:
                    raise bad("board", f"'++' in rank {r + 1}")
                prom = True
                continue
            if ch.isdigit():
                if prom or ch == "0":
                    raise bad("board", f"'{ch}' cannot stand there in rank {r + 1}")
                c += int(ch)
            else:
                t = _SFEN_TYPE.get(ch.upper()) if ch.isascii() and ch.isalpha() else None
                if t is None:
                    raise bad("board", f"unknown piece letter '{ch}' in rank {r + 1}")
                if prom and t not in _PROMOTABLE:
                    raise bad("board", f"'+{ch}' does not exist (rank {r + 1})")
                if c < 9:
                    board[r * 9 + c] = t | (0x10 if ch.islower() else 0) | (0x20 if prom else 0)
                c, prom = c + 1, False
            if c > 9:
                raise bad("board", f"rank {r + 1} holds more than 9 files")
        if prom:
            raise bad("board", f"'+' ends rank {r + 1}")
        if c != 9:
            raise bad("board", f"rank {r + 1} holds {c} files, expected 9")
    if parts[1] not in ("b", "w"):
        raise bad("side", f"'{parts[1]}' is neither 'b' nor 'w'")
    if parts[2] != "-":
        num = ""
        for ch in parts[2]:
            if ch.isdigit():
                num += ch
                continue
            t = _SFEN_TYPE.get(ch.upper()) if ch.isascii() and ch.isalpha() else None
            if t is None or t == 8:
                raise bad("hands", f"'{ch}' is no piece a hand can hold")
            cnt = int(num) if num else 1
            if cnt < 1 or cnt + int(hands[int(ch.islower()), t - 1]) > 255:
                raise bad("hands", f"count '{num}' before '{ch}'")
            hands[int(ch.islower()), t - 1] += cnt
            num = ""
        if num:
            raise bad("hands", f"count '{num}' without a piece")
    if len(parts) == 4 and not parts[3].isdigit():
        raise bad("move number", f"'{parts[3]}' is no number")
    return board, hands, int(parts[1] == "w")


_M64 = (1 << 64) - 1


def _mix64(x: np.ndarray) -> np.ndarray:
    """The splitmix64 finaliser of csrc/shogi_env.hip (mix64) over uint64 arrays."""
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def start_pool_index(seed: int, envs, games, count: int) -> np.ndarray:
    """Which pool row the game number `games` (0 = the one `reset()` starts) of env `envs` starts from, as the kernel
    draws it (include/keisei_amd.h): h = mix(seed ^ mix((env << 32 | g) + 0x706F6F6C)), idx = ((h >> 32) * count) >> 32.
    `envs` and `games` broadcast; returns int64."""
    if not 1 <= count < (1 << 31):
        raise ValueError(f"count must lie in [1, 2^31), got {count}")
    with np.errstate(over="ignore"):
        e = np.asarray(envs).astype(np.uint64) & np.uint64(0xFFFFFFFF)
        g = np.asarray(games).astype(np.uint64) & np.uint64(0xFFFFFFFF)
        h = _mix64(np.uint64(int(seed) & _M64) ^ _mix64(((e << np.uint64(32)) | g) + np.uint64(0x706F6F6C)))
        return (((h >> np.uint64(32)) * np.uint64(count)) >> np.uint64(32)).astype(np.int64)


def _valid_piece_table() -> np.ndarray:
    ok = np.zeros(256, bool)
    ok[0] = True
    for t in range(1, 9):
        for col in (0, 0x10):
            ok[t | col] = True
            if t in _PROMOTABLE:
                ok[t | col | 0x20] = True
    return ok


_VALID_PIECE = _valid_piece_table()


def _static_position_errors(boards: np.ndarray, hands: np.ndarray, sides: np.ndarray):
    """The checks of a start position that need no move generation, vectorised over K positions.  Returns (bad, why):
    `bad[k]` and the first failed check of position k."""
    K = boards.shape[0]
    why = np.full(K, "", dtype=object)
    bad = np.zeros(K, bool)

    def mark(cond: np.ndarray, text: str) -> None:
        new = cond & ~bad
        why[new] = text
        bad[:] |= cond

    mark(~_VALID_PIECE[boards].all(axis=1), "a board byte is no piece")
    mark(sides > 1, "side is neither 0 (black) nor 1 (white)")
    b = np.where(bad[:, None], 0, boards).astype(np.int64)     # rows already refused are not looked at further
    typ, white, prom = b & 15, (b & 0x10) != 0, (b & 0x20) != 0
    for col, name in ((0, "black"), (1, "white")):
        kings = ((typ == 8) & (white == bool(col))).sum(axis=1)
        mark(~bad & (kings != 1), f"{name} needs exactly one king")
    h = hands.reshape(K, 2, 7).astype(np.int64)
    for t in range(1, 8):
        total = (typ == t).sum(axis=1) + h[:, 0, t - 1] + h[:, 1, t - 1]
        mark(~bad & (total > _SET_MAX[t - 1]), f"more than {_SET_MAX[t - 1]} {_SFEN[t]} on the board and in the hands")
    rows = np.arange(81) // 9
    for col in (0, 1):
        last, last2 = (8, 7) if col else (0, 1)
        mine = (white == bool(col)) & ~prom
        dead = (mine & ((typ == 1) | (typ == 2)) & (rows == last)[None, :]).any(axis=1)
        mark(~bad & dead, "an unpromoted pawn or lance stands on its last rank")
        dead = (mine & (typ == 3) & ((rows == last) | (rows == last2))[None, :]).any(axis=1)
        mark(~bad & dead, "an unpromoted knight stands on its last two ranks")
        pawns = (mine & (typ == 1)).reshape(K, 9, 9).sum(axis=1)
        mark(~bad & (pawns > 1).any(axis=1), "two unpromoted pawns of one colour on a file")
    return bad, why


# ---------------------------------------------------------------------- spectator feed (spectator_data.rs)
# the move note of csrc/spectator.hip, from bit 0 (ka_spectator_words reports the same numbers)
NOTE_ACTION_BITS, NOTE_COLOUR, NOTE_TYPE, NOTE_PROMOTED, NOTE_DROP, NOTE_CAPTURE, NOTE_SUFFIX, NOTE_DISAMB, NOTE_NO_PIECE = \
    14, 14, 15, 19, 20, 21, 22, 24, 26
NOTE_WORDS = 1
_PIECE_NAMES = ("pawn", "lance", "knight", "silver", "gold", "bishop", "rook", "king")      # spectator_data.rs:45-56
_COLOR_NAMES = ("black", "white")
_SPECTATOR_KEYS = ("board", "hands", "current_player", "ply", "is_over", "result", "sfen", "in_check", "move_history")
_DIR_INDEX = {d: i for i, d in enumerate(_DIRS)}
_MAPPERS = (DefaultActionMapper(), SpatialActionMapper())


def _amode(action_mode) -> int:
    if action_mode in ("default", "spatial"):
        return int(action_mode == "spatial")
    if action_mode in (0, 1):
        return int(action_mode)
    raise ValueError(f"Unknown action_mode '{action_mode}'. Valid: 'default', 'spatial' (or 0, 1)")


def _square_hodges(sq: int) -> str:
    """spectator_data.rs:21-25: file (9 - column) and rank letter (row)."""
    return f"{9 - sq % 9}{'abcdefghi'[sq // 9]}"


def _decode_action(action: int, side: int, amode: int):
    """(from, to, promote, hand type or -1) of an action index on the real board, or None where it points off the board or
    lies outside the action space."""
    try:
        m = _MAPPERS[amode].decode(int(action), bool(side))
    except ValueError:
        return None
    if m["type"] == "drop":
        return m["to_sq"], m["to_sq"], False, m["piece_type_idx"]
    return m["from_sq"], m["to_sq"], m["promote"], -1


def host_move_note(board, side: int, mask_bits_row, action: int, action_mode) -> int:
    """The note kernel (`ka_spectator_note`, include/keisei_amd.h) restated on the host for one env: `board` the 81 piece
    bytes before the move, `side` the mover, `mask_bits_row` the packed legal mask the action is validated against."""
    amode, side = _amode(action_mode), int(side) & 1
    A = ACTION_SPACE if amode else DEFAULT_ACTION_SPACE
    action = int(action)
    if not 0 <= action < A:
        return 0
    mv = _decode_action(action, side, amode)
    if mv is None:
        return action
    board = np.asarray(board, np.uint8).reshape(81)
    row = np.ascontiguousarray(mask_bits_row).view(np.uint32).reshape(-1)
    frm, to, promote, drop = mv
    note = action | (side << NOTE_COLOUR)
    if drop >= 0:
        return note | ((drop + 1) << NOTE_TYPE) | (1 << NOTE_DROP)
    pc = int(board[frm])
    if board[to]:
        note |= 1 << NOTE_CAPTURE
    if not pc:
        return note | (1 << NOTE_NO_PIECE)
    t, prom = pc & 15, (pc >> 5) & 1
    from_row, to_row = frm // 9, to // 9
    if t in (1, 2):
        must = to_row == (8 if side else 0)
    elif t == 3:
        must = to_row >= 7 if side else to_row <= 1
    else:
        must = False
    zone = (from_row >= 6 or to_row >= 6) if side else (from_row <= 2 or to_row <= 2)
    suffix = 1 if (promote or must) else 2 if (not prom and t in _PROMOTABLE and zone) else 0
    flip = (lambda q: 80 - q) if side else (lambda q: q)
    to_p = flip(to)
    others = []
    if t != 8:
        for sq in range(81):
            if sq in (frm, to) or int(board[sq]) != pc:
                continue
            f_p = flip(sq)
            if amode:
                dr, dc = to_p // 9 - f_p // 9, to_p % 9 - f_p % 9
                if dr == 0 or dc == 0 or abs(dr) == abs(dc):
                    a0 = f_p * 139 + _DIR_INDEX[((dr > 0) - (dr < 0), (dc > 0) - (dc < 0))] * 8 + max(abs(dr), abs(dc)) - 1
                    a1 = a0 + 64
                elif dr == -2 and abs(dc) == 1:
                    a0 = f_p * 139 + 128 + (2 if dc > 0 else 0)
                    a1 = a0 + 1
                else:
                    continue
            else:
                a0 = f_p * 160 + (to_p - 1 if to_p > f_p else to_p) * 2
                a1 = a0 + 1
            if ((int(row[a0 >> 5]) >> (a0 & 31)) | (int(row[a1 >> 5]) >> (a1 & 31))) & 1:
                others.append(sq)
    if not others:
        disamb = 0
    elif not any(o % 9 == frm % 9 for o in others):
        disamb = 1
    elif not any(o // 9 == from_row for o in others):
        disamb = 2
    else:
        disamb = 3
    return note | (t << NOTE_TYPE) | (prom << NOTE_PROMOTED) | (suffix << NOTE_SUFFIX) | (disamb << NOTE_DISAMB)


def decode_move_note(note: int, action_mode) -> dict:
    """The fields of a move note.  `from_sq` / `to_sq` / `promote` come from the action index and the colour (`from_sq` is
    None for a drop); `valid` is False for a note that names no move (an action the env refuses)."""
    amode, note = _amode(action_mode), int(note) & 0xFFFFFFFF
    action, side = note & ((1 << NOTE_ACTION_BITS) - 1), (note >> NOTE_COLOUR) & 1
    d = {"action": action, "color": _COLOR_NAMES[side], "piece_type": (note >> NOTE_TYPE) & 15,
         "promoted": bool((note >> NOTE_PROMOTED) & 1), "drop": bool((note >> NOTE_DROP) & 1),
         "capture": bool((note >> NOTE_CAPTURE) & 1), "suffix": (note >> NOTE_SUFFIX) & 3,
         "disambiguation": (note >> NOTE_DISAMB) & 3, "no_piece": bool((note >> NOTE_NO_PIECE) & 1),
         "from_sq": None, "to_sq": None, "promote": False}
    mv = _decode_action(action, side, amode)
    d["valid"] = mv is not None and d["drop"] == (mv[3] >= 0) and (d["no_piece"] or 1 <= d["piece_type"] <= 8)
    if mv is not None:
        d["from_sq"], d["to_sq"], d["promote"] = (None if mv[3] >= 0 else mv[0]), mv[1], bool(mv[2])
    return d


def _hodges_of(d: dict) -> str:
    if not d["valid"]:
        return "?"
    to = _square_hodges(d["to_sq"])
    if d["drop"]:
        return f"{_SFEN[d['piece_type']]}*{to}"
    frm = d["from_sq"]
    if d["no_piece"]:
        return f"?{_square_hodges(frm)}-{to}"
    prefix = ("+" if d["promoted"] else "") + _SFEN[d["piece_type"]]
    dis = ("", str(9 - frm % 9), "abcdefghi"[frm // 9], _square_hodges(frm))[d["disambiguation"]]
    return f"{prefix}{dis}{'x' if d['capture'] else '-'}{to}{('', '+', '=', '')[d['suffix']]}"


def _usi_of(d: dict) -> str:
    if not d["valid"]:
        return "?"
    if d["drop"]:
        return f"{_SFEN[d['piece_type']]}*{_square_hodges(d['to_sq'])}"
    return _square_hodges(d["from_sq"]) + _square_hodges(d["to_sq"]) + ("+" if d["promote"] else "")


def hodges_notation(note: int, action_mode) -> str:
    """spectator_data.rs:109-186 from a move note: "P-7f", "Bx3c=", "Nx7c+", "+R-5a", "G6-5h", "Gf-5g", "S4g-5f", "P*5e";
    "?5e-5d" where no piece stood on the source square; "?" for a note that names no move."""
    return _hodges_of(decode_move_note(note, action_mode))


def move_usi(note: int, action_mode) -> str:
    """spectator_data.rs:93-103 from a move note: "7g7f", "8h2b+", "P*5e"; "?" for a note that names no move."""
    return _usi_of(decode_move_note(note, action_mode))


def move_history_entries(notes, action_mode) -> list:
    """The reference's `move_history` list (vec_env.rs:868-877) of one game from its notes."""
    out = []
    for n in notes:
        d = decode_move_note(int(n), action_mode)
        out.append({"action": d["action"], "notation": _hodges_of(d), "usi": _usi_of(d)})
    return out


def spectator_dicts(state_rows, histories=None, action_mode="spatial") -> list:
    """`build_spectator_dict` (spectator_data.rs:190-233) over env state rows on the host: `state_rows` (n, >= 104) uint8
    (board[81] hands[2][7] side in_check ... ply u32 at byte 100), `histories` one sequence of notes per row or None (empty
    histories).  The games of a VecEnv restart when they end, so `is_over` is False and `result` "in_progress"."""
    rows = np.ascontiguousarray(state_rows, dtype=np.uint8)
    if rows.ndim != 2 or rows.shape[1] < 104:
        raise ValueError(f"state_rows must have shape (n, >= 104), got {tuple(rows.shape)}")
    out = []
    for i, raw in enumerate(rows):
        board = []
        for sq in range(81):
            p = int(raw[sq])
            board.append(None if not p else {"type": _PIECE_NAMES[(p & 15) - 1], "color": _COLOR_NAMES[(p >> 4) & 1],
                                             "promoted": bool(p & 0x20), "row": sq // 9, "col": sq % 9})
        hands = {_COLOR_NAMES[c]: {_PIECE_NAMES[h]: int(raw[81 + c * 7 + h]) for h in range(7)} for c in (0, 1)}
        side = int(raw[95]) & 1
        out.append({"board": board, "hands": hands, "current_player": _COLOR_NAMES[side],
                    "ply": int(raw[100:104].view(np.uint32)[0]), "is_over": False, "result": "in_progress",
                    "sfen": format_sfen(raw[:81], raw[81:95], side), "in_check": bool(raw[96]),
                    "move_history": [] if histories is None else move_history_entries(histories[i], action_mode)})
    return out


@dataclass
class StepMetadata:          # step_result.rs:31-47
    captured_piece: Any
    termination_reason: Any
    ply_count: Any
    material_balance: Any


@dataclass
class StepResult:            # step_result.rs:50-83
    observations: Any
    legal_masks: Any
    rewards: Any
    terminated: Any
    truncated: Any
    terminal_observations: Any
    current_players: Any
    step_metadata: StepMetadata
    legal_mask_bits: Any = None      # (N, 352) int32 packed rows (torch output only): the device rollout store's column


@dataclass
class ResetResult:           # step_result.rs:86-97
    observations: Any
    legal_masks: Any
    legal_mask_bits: Any = None


class VecEnv:
    def __init__(self, num_envs: int = 512, max_ply: int = 500, observation_mode: str = "default",
                 action_mode: str = "default", *, device: Optional[torch.device] = None, output: str = "numpy",
                 check_actions: bool = True, start_pool_capacity: int = 0, move_history: bool = False):
        if observation_mode not in ("default", "katago"):
            raise ValueError(f"Unknown observation_mode '{observation_mode}'. Valid: 'default', 'katago'")
        if action_mode not in ("default", "spatial"):
            raise ValueError(f"Unknown action_mode '{action_mode}'. Valid: 'default', 'spatial'")
        self._omode, self._amode = int(observation_mode == "katago"), int(action_mode == "spatial")
        self._A = ACTION_SPACE if self._amode else DEFAULT_ACTION_SPACE
        self._C = OBS_CHANNELS if self._omode else DEFAULT_OBS_CHANNELS
        if output not in ("numpy", "torch"):
            raise ValueError("output must be 'numpy' or 'torch'")
        if num_envs <= 0 or max_ply < 0 or max_ply > 65535:
            raise ValueError("num_envs must be positive and 0 <= max_ply <= 65535")
        if start_pool_capacity < 0 or start_pool_capacity >= (1 << 31):
            raise ValueError(f"start_pool_capacity must lie in [0, 2^31), got {start_pool_capacity}")
        _lib._load()                                          # raises KeiseiHipError when the library is missing
        if not torch.cuda.is_available():
            raise _lib.KeiseiHipError("keisei_amd.shogi_gym.VecEnv needs a GPU (there is no CPU fallback)")
        self.device = torch.device(device if device is not None else f"cuda:{torch.cuda.current_device()}")
        self._n, self._max_ply, self._output, self._check = int(num_envs), int(max_ply), output, bool(check_actions)
        n, dev, hist = self._n, self.device, max(self._max_ply, 1)
        z = lambda *shape, dtype: torch.zeros(*shape, dtype=dtype, device=dev)
        self._state = z(n, _lib.query("ka_shogi_env_state_bytes"), dtype=torch.uint8)
        self._keys = z(n, hist, dtype=torch.int64)
        self._checks = z(n, hist, dtype=torch.uint8)
        self._obs = [z(n, self._C, 9, 9, dtype=torch.float32) for _ in range(2)]
        self._mask = [z(n, self._A, dtype=torch.bool) for _ in range(2)]
        self._bits = [z(n, (self._A + 31) // 32, dtype=torch.int32) for _ in range(2)]
        self._cur = 0
        two = lambda *shape, dtype: [z(*shape, dtype=dtype) for _ in range(2)]
        self._rewards = two(n, dtype=torch.float32)
        self._terminated = two(n, dtype=torch.bool)
        self._truncated = two(n, dtype=torch.bool)
        # ONE persistent buffer, as the reference's terminal_obs_buffer (vec_env.rs:246,598): a game's row is rewritten only
        # when that game ends again, rows of running games keep what they held
        self._terminal_obs = z(n, self._C, 9, 9, dtype=torch.float32)
        self._players = two(n, dtype=torch.uint8)
        self._captured = [torch.full((n,), 255, dtype=torch.uint8, device=dev) for _ in range(2)]
        self._reason = two(n, dtype=torch.uint8)
        self._ply = two(n, dtype=torch.int16)                 # u16 payload (max_ply <= 65535); viewed as uint16 on the host
        self._material = two(n, dtype=torch.int32)
        self._stats = z(4, dtype=torch.int64)
        self._err = z(2, dtype=torch.int64)                   # [this step's refusal, the latch raise_if_refused reads and clears]
        self._actions = z(n, dtype=torch.int64)
        self._mate: dict = {}                                 # mate_in_one's / mate_in_three's scratch rows by caps, allocated at the first call
        self._perft: dict = {}                                # perft's rows by (depth, rows), allocated at the first call
        # start positions (set_start_positions): allocated once, so that a captured graph keeps valid pointers; the
        # header {count, 0, seed lo, seed hi} is read by every launch.  Capacity 0: no pool, the entry points without one.
        self._pool_capacity = int(start_pool_capacity)
        self._pool = self._pool_hdr = None
        if self._pool_capacity:
            self._pool = z(self._pool_capacity, POOL_ROW_BYTES, dtype=torch.uint8)
            self._pool_hdr = z(4, dtype=torch.int32)
        # move histories (move_history=True): a note per move of the game in progress (csrc/spectator.hip), allocated once
        self._hist = self._hist_count = self._hist_pending = None
        if move_history:
            self._hist = z(n, hist, dtype=torch.int32)
            self._hist_count = z(n, dtype=torch.int32)
            self._hist_pending = z(n, dtype=torch.int32)
        # as in the reference's constructor (vec_env.rs:574-612): the games stand at the start position, the mask buffer
        # is still all-false -- a step() before reset() is refused ("action index ... is not legal")
        self.reset()
        for t in (self._obs[0], self._mask[0], self._bits[0]):
            t.zero_()
        self._armed = False

    # ------------------------------------------------------------------ core
    def reset(self) -> ResetResult:
        """vec_env.rs:617-645: every game back to the start position; observations and masks of the first move."""
        self._armed = True
        with torch.cuda.device(self.device):
            self._cur = 0
            self._err.zero_()                                 # (a refusal nobody asked about ends with the games it belonged to)
            self._call_reset(self._obs[0], self._mask[0], self._bits[0], self._players[0], 0)
            self._clear_histories()
        return ResetResult(self._out(self._obs[0]), self._out(self._mask[0]),
                           self._bits[0] if self._output == "torch" else None)

    def step(self, actions) -> StepResult:
        """vec_env.rs:651-790.  `actions`: N action indices (list, numpy array or tensor; a CUDA int64 tensor is used in place)."""
        n = self._n
        if isinstance(actions, torch.Tensor):
            if actions.numel() != n:
                raise ValueError(f"expected {n} actions, got {actions.numel()}")
            act = actions.reshape(n)
            if act.device != self.device or act.dtype != torch.int64 or not act.is_contiguous():
                self._actions.copy_(act.to(torch.int64), non_blocking=True)
                act = self._actions
        else:
            a = np.asarray(actions, dtype=np.int64).reshape(-1)
            if a.shape[0] != n:
                raise ValueError(f"expected {n} actions, got {a.shape[0]}")
            self._actions.copy_(torch.from_numpy(a), non_blocking=False)
            act = self._actions
        if not getattr(self, "_armed", True):                 # no masks were handed out yet: every action is refused
            a0 = int(act[0].item())
            if a0 < 0:
                raise ValueError(f"env 0: negative action index {a0}")
            raise RuntimeError(f"env 0: action index {a0} is not legal")
        prev, nxt = self._cur, self._cur ^ 1
        with torch.cuda.device(self.device):
            args = (self._state, self._keys, self._checks, act, n, self._max_ply, self._omode, self._amode,
                    self._mask[prev], self._bits[prev], self._err, self._obs[nxt], self._mask[nxt], self._bits[nxt],
                    self._rewards[nxt], self._terminated[nxt], self._truncated[nxt], self._terminal_obs, self._players[nxt],
                    self._captured[nxt], self._reason[nxt], self._ply[nxt], self._material[nxt], self._stats)
            if self._hist is not None:                        # the move's note, from the position and the mask before it
                _lib.call("ka_spectator_note", self._state, self._state.shape[1], n, self._bits[prev], act, self._amode,
                          self._hist_pending, _lib.stream_ptr())
            if self._pool is None:
                _lib.call("ka_shogi_env_step", *args, _lib.stream_ptr())
            else:
                _lib.call("ka_shogi_env_step_pool", *args, self._pool, self._pool_hdr, _lib.stream_ptr())
            if self._hist is not None:                        # appended unless the step was refused; finished games cleared
                _lib.call("ka_spectator_commit", self._err, self._terminated[nxt], self._truncated[nxt], n,
                          self._hist_pending, self._hist, self._hist.shape[1], self._hist_count, _lib.stream_ptr())
        self._cur = nxt                                       # (a refused step has re-written the unchanged positions there)
        if self._check:
            self.raise_if_refused(act)
        o = self._out
        ply = self._ply[nxt] if self._output == "torch" else self._ply[nxt].cpu().numpy().view(np.uint16)
        meta = StepMetadata(o(self._captured[nxt]), o(self._reason[nxt]), ply, o(self._material[nxt]))
        return StepResult(o(self._obs[nxt]), o(self._mask[nxt]), o(self._rewards[nxt]), o(self._terminated[nxt]),
                          o(self._truncated[nxt]), o(self._terminal_obs), o(self._players[nxt]), meta,
                          self._bits[nxt] if self._output == "torch" else None)

    def raise_if_refused(self, actions: Optional[torch.Tensor] = None) -> None:
        """The reference refuses a step before anything moves (vec_env.rs:660-690); so does the kernel, and this reads
        its latch (one 8-byte copy).  With check_actions=False call it whenever convenient: a refused step moved no game,
        its result holds the unchanged positions again (zero rewards, no flags), and the latch keeps the FIRST refusal --
        env index and action, stored by the kernel -- through any number of later steps until it is reported here."""
        word = int(self._err[1].item())
        if word == 0:
            return
        self._err[1].zero_()
        i = self._n - (word >> 32)
        a = word & 0xFFFFFFFF
        a = a - (1 << 32) if a >= (1 << 31) else a
        if actions is not None and abs(a) >= (1 << 31) - 1:   # clamped by the kernel: the caller's own tensor has the exact index
            a = int(actions[i].item())
        if a < 0:
            raise ValueError(f"env {i}: negative action index {a}")
        raise RuntimeError(f"env {i}: action index {a} is not legal")

    def _out(self, t: torch.Tensor):
        return t if self._output == "torch" else t.cpu().numpy()

    def _clear_histories(self) -> None:
        if self._hist is not None:
            _lib.call("ka_spectator_begin", self._hist_count, self._n, _lib.stream_ptr())

    def _call_reset(self, obs, mask, bits, players, refresh: int) -> None:
        args = (self._state, self._keys, self._checks, self._n, self._max_ply, self._omode, self._amode, obs, mask, bits,
                players, refresh)
        if self._pool is None:
            _lib.call("ka_shogi_env_reset", *args, _lib.stream_ptr())
        else:
            _lib.call("ka_shogi_env_reset_pool", *args, self._pool, self._pool_hdr, _lib.stream_ptr())

    # ------------------------------------------------------------------ properties (vec_env.rs:793-870)
    @property
    def action_space_size(self) -> int:
        return self._A

    @property
    def observation_channels(self) -> int:
        return self._C

    @property
    def num_envs(self) -> int:
        return self._n

    def _stat(self, i: int) -> int:
        return int(self._stats[i].item())

    @property
    def episodes_completed(self) -> int:
        return self._stat(0)

    @property
    def episodes_drawn(self) -> int:
        return self._stat(1)

    @property
    def episodes_truncated(self) -> int:
        return self._stat(2)

    @property
    def draw_rate(self) -> float:
        c = self._stat(0)
        return 0.0 if c == 0 else self._stat(1) / c

    @property
    def mean_episode_length(self) -> float:
        c = self._stat(0)
        return 0.0 if c == 0 else self._stat(3) / c

    @property
    def truncation_rate(self) -> float:
        c = self._stat(0)
        return 0.0 if c == 0 else self._stat(2) / c

    def reset_stats(self) -> None:
        self._stats.zero_()

    # ------------------------------------------------------------------ positions
    def get_state(self, game_id: int):
        """(board[81] piece bytes, hands[2][7], side to move, ply) of one game (piece bytes: piece.rs:10-19)."""
        if not 0 <= game_id < self._n:
            raise IndexError(f"game_id {game_id} out of range for {self._n} environments")
        raw = self._state[game_id].cpu().numpy()
        return raw[:81].copy(), raw[81:95].reshape(2, 7).copy(), int(raw[95]), int(raw[100:104].view(np.uint32)[0])

    def set_state(self, game_id: int, board, hands, side: int) -> None:
        """Place a position in one game (ply and history restart at 0) and refresh every game's observation and masks --
        the rule fixtures of the reference's tests build their positions square by square (rules.rs:575-1790)."""
        others = [self.get_state(i) for i in range(self._n) if i != game_id]
        if any(p != 0 for *_, p in others):
            raise RuntimeError("set_state refreshes all games from ply 0: call it right after reset()")
        raw = self._state.cpu().numpy()
        raw[game_id, :81] = np.asarray(board, np.uint8).reshape(81)
        raw[game_id, 81:95] = np.asarray(hands, np.uint8).reshape(14)
        raw[game_id, 95] = side
        self._refresh(raw)

    def set_states(self, boards, hands, sides) -> None:
        """All games at once: boards (N,81), hands (N,2,7) or (N,14), sides (N,); ply and history restart at 0."""
        raw = np.zeros(tuple(self._state.shape), np.uint8)
        if self._pool is not None:                            # the count of games started is not a part of the position
            raw[:, 116:120] = self._state[:, 116:120].cpu().numpy()
        raw[:, :81] = np.asarray(boards, np.uint8).reshape(self._n, 81)
        raw[:, 81:95] = np.asarray(hands, np.uint8).reshape(self._n, 14)
        raw[:, 95] = np.asarray(sides, np.uint8).reshape(self._n)
        self._refresh(raw)

    def _refresh(self, raw: np.ndarray) -> None:
        self._armed = True
        self._state.copy_(torch.from_numpy(raw))
        with torch.cuda.device(self.device):
            self._call_reset(self._obs[self._cur], self._mask[self._cur], self._bits[self._cur], self._players[self._cur], 1)
            self._clear_histories()

    # ------------------------------------------------------------------ start positions
    @property
    def start_pool_capacity(self) -> int:
        return self._pool_capacity

    @property
    def start_pool_count(self) -> int:
        """How many start positions are in use (0: every game starts at the standard position)."""
        return 0 if self._pool_hdr is None else int(self._pool_hdr[0].item())

    def _probe_positions(self, boards: np.ndarray, hands: np.ndarray, sides: np.ndarray):
        """(side to move is in check, it has a legal move) of K positions, by refresh launches over scratch rows."""
        K = boards.shape[0]
        in_check, movable = np.zeros(K, bool), np.zeros(K, bool)
        dev, chunk = self.device, 1024
        words = (self._A + 31) // 32
        with torch.cuda.device(dev):
            m = min(K, chunk)
            state = torch.zeros(m, self._state.shape[1], dtype=torch.uint8, device=dev)
            keys = torch.zeros(m, max(self._max_ply, 1), dtype=torch.int64, device=dev)
            checks = torch.zeros(m, max(self._max_ply, 1), dtype=torch.uint8, device=dev)
            obs = torch.zeros(m, self._C, 9, 9, dtype=torch.float32, device=dev)
            bits = torch.zeros(m, words, dtype=torch.int32, device=dev)
            for lo in range(0, K, chunk):
                k = min(chunk, K - lo)
                raw = np.zeros((k, state.shape[1]), np.uint8)
                raw[:, :81], raw[:, 81:95], raw[:, 95] = boards[lo:lo + k], hands[lo:lo + k], sides[lo:lo + k]
                state[:k].copy_(torch.from_numpy(raw))
                _lib.call("ka_shogi_env_reset", state, keys, checks, k, self._max_ply, self._omode, self._amode, obs, None,
                          bits, None, 1, _lib.stream_ptr())
                in_check[lo:lo + k] = state[:k, 96].cpu().numpy() != 0
                movable[lo:lo + k] = (bits[:k] != 0).any(dim=1).cpu().numpy()
        return in_check, movable

    def set_start_positions(self, boards, hands, sides, *, seed: int = 0) -> None:
        """Start every later game -- the restarts inside `step` and the games of `reset()` -- from one of these K
        positions: boards (K,81) piece bytes, hands (K,2,7) or (K,14), sides (K,), host arrays or tensors.  The game
        number g (0 at `reset()`) of env e starts from row `start_pool_index(seed, e, g, K)`, with ply 0 and an empty
        history.  Games in progress go on; a captured graph needs no new capture.  The positions are validated first
        (a `ValueError` names the first bad index and nothing is uploaded): the kernel assumes playable positions."""
        to_np = lambda x: x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)  # noqa: E731
        b, h, s = to_np(boards), to_np(hands), to_np(sides)
        if b.ndim != 2 or b.shape[1] != 81:
            raise ValueError(f"boards must have shape (K, 81), got {tuple(b.shape)}")
        K = b.shape[0]
        if tuple(h.shape) not in ((K, 2, 7), (K, 14)) or s.reshape(-1).shape[0] != K or s.ndim > 1:
            raise ValueError(f"hands must have shape ({K}, 2, 7) or ({K}, 14) and sides ({K},), got {tuple(h.shape)} "
                             f"and {tuple(s.shape)}")
        if self._pool_capacity == 0:
            raise ValueError("this VecEnv has no start pool: construct it with start_pool_capacity > 0")
        if K > self._pool_capacity:
            raise ValueError(f"{K} start positions do not fit start_pool_capacity={self._pool_capacity}")
        if K == 0:
            raise ValueError("no start positions given (clear_start_positions() returns to the standard start)")
        for name, x in (("boards", b), ("hands", h), ("sides", s)):
            if x.dtype.kind not in "iub" or (x.size and (int(x.min()) < 0 or int(x.max()) > 255)):
                raise ValueError(f"{name} must hold integers in [0, 255]")
        b, h, s = (np.ascontiguousarray(x, dtype=np.uint8) for x in (b, h.reshape(K, 14), s.reshape(K)))
        bad, why = _static_position_errors(b, h, s)
        first = int(np.argmax(bad)) if bad.any() else K
        if first:                                             # the rows before the first refused one go to the device
            mover_checked, movable = self._probe_positions(b[:first], h[:first], s[:first])
            other_checked, _ = self._probe_positions(b[:first], h[:first], s[:first] ^ 1)
            dyn = other_checked | ~movable
            if dyn.any():
                first = int(np.argmax(dyn))
                reason = "the side not to move is in check" if other_checked[first] else "the side to move has no legal move"
                raise ValueError(f"start position {first} is not playable: {reason}")
        if first < K:
            raise ValueError(f"start position {first} is not playable: {why[first]}")
        rows = np.concatenate([b, h, s[:, None]], axis=1)
        sd = int(seed) & _M64
        hdr = np.array([K, 0, sd & 0xFFFFFFFF, sd >> 32], dtype=np.uint32).view(np.int32)
        with torch.cuda.device(self.device):
            # in stream order behind the launches queued so far: rows and seed first, the count that exposes them last
            self._pool[:K].copy_(torch.from_numpy(rows))
            self._pool_hdr.copy_(torch.from_numpy(hdr))

    def set_start_sfens(self, sfens, *, seed: int = 0) -> None:
        """`set_start_positions` of SFEN strings (`parse_sfen`)."""
        parsed = [parse_sfen(x) for x in sfens]
        if not parsed:
            raise ValueError("no start positions given (clear_start_positions() returns to the standard start)")
        self.set_start_positions(np.stack([p[0] for p in parsed]), np.stack([p[1] for p in parsed]),
                                 np.asarray([p[2] for p in parsed], np.uint8), seed=seed)

    def clear_start_positions(self) -> None:
        """Later games start at the standard position again (count 0); games in progress go on."""
        if self._pool_hdr is not None:
            with torch.cuda.device(self.device):
                self._pool_hdr.zero_()

    def current(self) -> ResetResult:
        """Observation and masks of the positions to move (what the last reset / step / set_state wrote)."""
        c = self._cur
        return ResetResult(self._out(self._obs[c]), self._out(self._mask[c]), self._bits[c] if self._output == "torch" else None)

    def mate_in_one(self, max_checks: int = 32):
        """Does the side to move have a mate in one?  `(actions, n_checks, truncated)`, (N,) int64 tensors on the env's
        device for the positions now to move: the mating action with the lowest index or -1, the number of legal moves
        that give check, and 1 where more than `max_checks` (1..64) of them exist -- only the first `max_checks` in
        ascending action order are tried, so a -1 beside a 1 is no proof.  Three stages (`training/mate_search.py`,
        csrc/mate.hip): the checking moves are forked into scratch rows, stepped by the env's own step kernel, and a row
        that ended by checkmate names the move.  The env is only read: calling it twice gives the same answer.  For
        katago / spatial envs; any other mode raises `ValueError`."""
        from keisei_amd.training.mate_search import FLAG_MATE, FLAG_TRUNCATED, REC_ACTION, REC_FLAGS, REC_NCHECKS, \
            MateControls, MateSearch, mate_table
        if self._omode != 1 or self._amode != 1:
            raise ValueError("mate_in_one covers the katago observation and the spatial action mode only")
        cap = MateControls(max_checks).max_checks
        if cap < 1:
            raise ValueError(f"max_checks must be an integer in [1, 64], got {max_checks!r}")
        with torch.cuda.device(self.device):
            ms = self._mate.get(cap)
            if ms is None:                                    # the scratch rows of this cap, allocated at the first call
                # (a weak reference back: no cycle, so the rows and the pinned counters die with the env, at once)
                ms = self._mate[cap] = (MateSearch(weakref.proxy(self), cap), torch.from_numpy(mate_table(MateControls(cap), 1)).to(self.device),
                                        torch.zeros(self._n, dtype=torch.int32, device=self.device))
            search, table, model_of = ms
            # the unused slots replay a legal move of the position: its first
            actions = self._mask[self._cur].to(torch.uint8).argmax(dim=1)
            search.clear()
            search.step(self._bits[self._cur], actions, model_of, table, _lib.stream_ptr())
            search.read()                                     # raises on the error word
            rec = search.records().to(torch.int64)
        flags = rec[:, REC_FLAGS]
        mate = torch.where((flags & FLAG_MATE) != 0, rec[:, REC_ACTION], torch.full_like(flags, -1))
        return mate, rec[:, REC_NCHECKS], ((flags & FLAG_TRUNCATED) != 0).to(torch.int64)

    def mate_records(self, max_checks: int = 32) -> torch.Tensor:
        """The (N, 4 + max_checks) int32 records of the last `mate_in_one(max_checks)` (csrc/mate.hip: flags, number of
        checking moves, slot, action, the checking actions forked)."""
        ms = self._mate.get(int(max_checks))
        if ms is None:
            raise ValueError(f"mate_in_one(max_checks={max_checks}) has not been called on this env")
        return ms[0].records()

    def _mate3_search(self, max_checks, evasion_rows, reply_checks):
        from keisei_amd.training.mate_search import Mate3Search, MateControls, mate3_reply_table, mate_table
        if self._omode != 1 or self._amode != 1:
            raise ValueError("mate_in_three covers the katago observation and the spatial action mode only")
        ctl = MateControls(max_checks, 0, evasion_rows, reply_checks)
        if ctl.max_checks < 1 or ctl.evasion_rows < 1:
            raise ValueError(f"max_checks, evasion_rows and reply_checks must be positive, got {max_checks!r}, "
                             f"{evasion_rows!r} and {reply_checks!r}")
        key = (ctl.max_checks, ctl.evasion_rows, ctl.reply_checks)
        ms = self._mate.get(key)
        if ms is None:                                        # the scratch rows of these caps, allocated at the first call
            table = mate_table(ctl, 1)
            ms = self._mate[key] = (Mate3Search(weakref.proxy(self), *key), torch.from_numpy(table).to(self.device),
                                    torch.from_numpy(mate3_reply_table(table)).to(self.device),
                                    torch.zeros(self._n, dtype=torch.int32, device=self.device))
        return ms

    def mate_in_three(self, max_checks: int = 16, evasion_rows: int = 32, reply_checks: int = 8):
        """Does the side to move have a mate in one, or a forced mate in three?  `(actions, depth, cut)`, (N,) int64
        tensors on the env's device for the positions now to move: the mating move or -1; 1 for a mate in one (the move
        `mate_in_one` gives), 3 for a mate in three (the lowest checking move after which every reply runs into a mate in
        one), 0 for neither; and 1 where a cap cut the search -- more than `max_checks` (1..64) checking moves, a check
        whose evasions did not fit what was left of the `evasion_rows` (1..128) grandchild rows, or a reply without a
        mate among its first `reply_checks` (1..64) checking moves when it has more -- so a 0 beside a 1 is no proof.  A
        mate that is found is always one.  The stages are those of `training/mate_search.py` (csrc/mate.hip,
        csrc/mate3.hip); the env is only read.  For katago / spatial envs; any other mode raises `ValueError`."""
        from keisei_amd.training.mate_search import FLAG3_MATE, FLAG3_REPLY_TRUNCATED, FLAG3_SKIPPED, FLAG_MATE, \
            FLAG_TRUNCATED, REC3_ACTION, REC3_FLAGS, REC_ACTION, REC_FLAGS
        with torch.cuda.device(self.device):
            search, table, reply_table, model_of = self._mate3_search(max_checks, evasion_rows, reply_checks)
            # the unused slots replay a legal move of the position: its first
            actions = self._mask[self._cur].to(torch.uint8).argmax(dim=1)
            search.clear()
            search.step(self._bits[self._cur], actions, model_of, table, reply_table, _lib.stream_ptr())
            search.root.read()                                # raise on the error words
            search.read()
            rec1, rec3 = search.root.records().to(torch.int64), search.records().to(torch.int64)
        f1, f3 = rec1[:, REC_FLAGS], rec3[:, REC3_FLAGS]
        one, three = (f1 & FLAG_MATE) != 0, (f3 & FLAG3_MATE) != 0
        none = torch.full_like(f1, -1)
        move = torch.where(one, rec1[:, REC_ACTION], torch.where(three, rec3[:, REC3_ACTION], none))
        depth = torch.where(one, torch.ones_like(f1), torch.where(three, torch.full_like(f1, 3), torch.zeros_like(f1)))
        cut = ((f1 & FLAG_TRUNCATED) != 0) | ((f3 & (FLAG3_SKIPPED | FLAG3_REPLY_TRUNCATED)) != 0)
        return move, depth, cut.to(torch.int64)

    def mate3_records(self, max_checks: int = 16, evasion_rows: int = 32, reply_checks: int = 8):
        """`(root, deep)` of the last `mate_in_three` with these caps: the (N, 4 + max_checks) int32 mate-in-one records
        (csrc/mate.hip) and the (N, 6 + 2 * max_checks) int32 mate-in-three records (csrc/mate3.hip: flags, grandchild
        rows used, slot, action, the proving set, every slot's evasion count and first row)."""
        ms = self._mate.get((int(max_checks), int(evasion_rows), int(reply_checks)))
        if ms is None:
            raise ValueError(f"mate_in_three({max_checks}, {evasion_rows}, {reply_checks}) has not been called on this env")
        return ms[0].root.records(), ms[0].records()

    def _perft_walk(self, depth, rows):
        from keisei_amd.perft import PerftWalk, check_perft_args
        if self._omode != 1 or self._amode != 1:
            raise ValueError("perft covers the katago observation and the spatial action mode only")
        key = check_perft_args(depth, rows)
        walk = self._perft.get(key)
        if walk is None:                                      # the rows of this (depth, rows), allocated at the first call
            walk = self._perft[key] = PerftWalk(weakref.proxy(self), *key)
        return walk

    def perft(self, depth: int, rows: int = 16384, bulk: bool = True):
        """Count the game tree beneath the N positions now to move, to `depth` (1..8) plies: a `PerftResult` of host
        `np.uint64` arrays -- `nodes` (N,) the leaves per env, `by_depth` (N, depth, 4) per depth the nodes, the nodes ended
        by checkmate, the nodes ended otherwise and the nodes whose side to move is in check, `chunks` the number of fork
        launches.  Every legal move of a frontier of positions is forked into a scratch row and stepped by the env's own
        step kernel (keisei_amd/perft.py, csrc/perft.hip); a level of the walk holds at most `rows` rows (1..2^20, and at
        least the most moves any position in the tree has -- 593 always suffices -- or a `ValueError` names the row), so a
        small `rows` only splits the work into more chunks.  With `bulk=True` the last depth is counted from the masks of
        the depth before it and carries nodes only (zeros in the other columns); with `bulk=False` it is forked and
        stepped too.  This is perft under the env's game rules: a position in which the game has ended has no successors
        (the step restarts such a row).  It equals the move-generation perft of a rules engine (the oracle's `so_perft`)
        wherever no game in the tree ends other than by checkmate; the "ended otherwise" column says when that fails.  The
        env is only read.  For katago / spatial envs; any other mode, `depth` or `rows` raises `ValueError`."""
        return self._perft_walk(depth, rows).perft(int(depth), bool(bulk))

    def perft_divide(self, depth: int, rows: int = 16384) -> List[dict]:
        """Per env a dict from each legal action to the leaf count beneath it at `depth`: the values of env e sum to
        `perft(depth).nodes[e]`, which is what narrows a wrong count down to a position.  Arguments and meaning as `perft`."""
        return self._perft_walk(depth, rows).divide(int(depth))

    def get_sfen(self, game_id: int) -> str:
        """vec_env.rs:873-882 / sfen.rs:93-171."""
        board, hands, side, _ = self.get_state(game_id)
        return format_sfen(board, hands, side)

    def get_sfens(self) -> List[str]:
        return [self.get_sfen(i) for i in range(self._n)]

    @property
    def move_history(self) -> bool:
        """Whether the env keeps the move notes of the games in progress (`VecEnv(..., move_history=True)`)."""
        return self._hist is not None

    def move_notes(self, game_ids=None) -> List[np.ndarray]:
        """The notes (uint32, `decode_move_note`) of the moves of the games in progress, one array per env (or per
        requested id), read in one copy; empty arrays without `move_history=True`."""
        ids = self._game_ids(game_ids)
        if self._hist is None:
            return [np.zeros(0, np.uint32) for _ in ids]
        both = torch.cat([self._hist_count[:, None], self._hist], dim=1)
        if game_ids is not None:
            both = both[torch.as_tensor(ids, dtype=torch.int64, device=self.device)]
        both = both.cpu().numpy()
        return [both[j, 1:1 + max(0, min(int(both[j, 0]), both.shape[1] - 1))].copy().view(np.uint32) for j in range(len(ids))]

    def _game_ids(self, game_ids) -> List[int]:
        if game_ids is None:
            return list(range(self._n))
        ids = [int(i) for i in game_ids]
        for i in ids:
            if not 0 <= i < self._n:
                raise IndexError(f"game_id {i} out of range for {self._n} environments")
        return ids

    def get_spectator_data(self, game_ids=None) -> List[dict]:
        """vec_env.rs:862-882 / spectator_data.rs:190-233: one dict per env (or per requested id) with the keys `board`,
        `hands`, `current_player`, `ply`, `is_over`, `result`, `sfen`, `in_check`, `move_history`.  The state rows are read
        in one copy and, with `move_history=True`, the notes in one more; without it `move_history` is []."""
        ids = self._game_ids(game_ids)
        rows = self._state if game_ids is None else self._state[torch.as_tensor(ids, dtype=torch.int64, device=self.device)]
        notes = self.move_notes(game_ids) if self._hist is not None else None
        return spectator_dicts(rows.cpu().numpy(), notes, self._amode)
