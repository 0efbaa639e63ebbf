"""The spectator feed on the host: the move note restated in numpy (`host_move_note`) and its text (`hodges_notation`,
`move_usi`) against the known answers of the reference's own notation tests (spectator_data.rs:244-727, restated as data in
tests/golden/g16_spectator_vectors.json), the
full-square disambiguation the reference's vectors never reach, an independent restatement of `move_notation` over oracle
playouts, and the dict builder of `get_spectator_data` against the reference's test_vec_env.py."""
import json
import re
from functools import lru_cache
from pathlib import Path

import numpy as np
import pytest

from keisei_amd import _lib
from keisei_amd import shogi_gym as G
from keisei_amd.shogi_gym import (DefaultActionMapper, SpatialActionMapper, decode_move_note, format_sfen, hodges_notation,
                                  host_move_note, move_usi, parse_sfen, spectator_dicts)
from oracle import shogi as so
from start_pool_helpers import START

GOLDEN = Path(__file__).resolve().parent / "golden"

TYPES = {"P": 1, "L": 2, "N": 3, "S": 4, "G": 5, "B": 6, "R": 7, "K": 8}
MODES = (("spatial", 1), ("default", 0))
PLAY_SEED = 3         # with it the playouts below meet a capture, a drop, '+', '=', a promoted mover and a disambiguation


@lru_cache(maxsize=None)
def vectors():
    return json.loads((GOLDEN / "g16_spectator_vectors.json").read_text())["vectors"]


def vector_board(v, kings: bool = False) -> np.ndarray:
    b = np.zeros(81, np.uint8)
    for r, c, t, col, prom in v["pieces"]:
        b[r * 9 + c] = TYPES[t] | (0x10 if col == "white" else 0) | (0x20 if prom else 0)
    if kings:
        for col, (r, c) in v["kings"].items():
            b[r * 9 + c] = 8 | (0x10 if col == "white" else 0)
    return b


def vector_hands(v) -> np.ndarray:
    return np.array([v["hands"]["black"], v["hands"]["white"]], np.uint8)


def move_action(m, side: int, spatial: int) -> int:
    mapper = SpatialActionMapper() if spatial else DefaultActionMapper()
    to = m["to"][0] * 9 + m["to"][1]
    if "drop" in m:
        return mapper.encode_drop_move(to, "PLNSGBR".index(m["drop"]), bool(side))
    return mapper.encode_board_move(m["from"][0] * 9 + m["from"][1], to, bool(m["promote"]), bool(side))


def pack_row(actions, spatial: int) -> np.ndarray:
    A = G.ACTION_SPACE if spatial else G.DEFAULT_ACTION_SPACE
    row = np.zeros((A + 31) // 32, np.uint32)
    for a in actions:
        row[a >> 5] |= np.uint32(1 << (a & 31))
    return row


def pack_mask(mask: np.ndarray) -> np.ndarray:
    return np.packbits(np.concatenate([mask.astype(bool), np.zeros((-len(mask)) % 32, bool)]), bitorder="little").view(np.uint32)


# ------------------------------------------------------------------ layout
def test_note_layout_matches_the_library():
    names = ("NOTE_ACTION_BITS", "NOTE_COLOUR", "NOTE_TYPE", "NOTE_PROMOTED", "NOTE_DROP", "NOTE_CAPTURE", "NOTE_SUFFIX",
             "NOTE_DISAMB", "NOTE_NO_PIECE", "NOTE_WORDS")
    for which, name in enumerate(names):
        assert _lib.query("ka_spectator_words", which) == getattr(G, name), name
    assert _lib.query("ka_spectator_words", len(names)) == -1 and _lib.query("ka_spectator_words", -1) == -1
    assert (1 << G.NOTE_ACTION_BITS) > G.DEFAULT_ACTION_SPACE > G.ACTION_SPACE


# ------------------------------------------------------------------ names, squares, zones (spectator_data.rs:244-374)
def test_names_squares_and_promotion_zones():
    assert G._PIECE_NAMES == ("pawn", "lance", "knight", "silver", "gold", "bishop", "rook", "king")
    assert G._COLOR_NAMES == ("black", "white")
    assert [G._SFEN[t] for t in range(1, 9)] == list("PLNSGBRK")
    assert [G._square_hodges(s) for s in (0, 80, 40, 8, 72)] == ["9a", "1i", "5e", "1a", "9i"]

    def suffix(piece, frm, to, side=0):
        board = np.zeros(81, np.uint8)
        board[frm] = piece
        a = SpatialActionMapper().encode_board_move(frm, to, False, bool(side))
        return decode_move_note(host_move_note(board, side, pack_row([a], 1), a, 1), 1)["suffix"]

    assert suffix(4, 5 * 9 + 4, 4 * 9 + 4) == 0 and suffix(4, 3 * 9 + 4, 2 * 9 + 4) == 2      # silver outside / into the zone
    assert suffix(4, 2 * 9 + 4, 3 * 9 + 3) == 2                                              # out of the zone
    assert suffix(5, 3 * 9 + 4, 2 * 9 + 4) == 0 and suffix(8, 3 * 9 + 4, 2 * 9 + 4) == 0      # gold, king
    assert suffix(4 | 0x20, 3 * 9 + 4, 2 * 9 + 4) == 0                                       # already promoted
    for row in range(9):                                                                     # the zones: rows 0-2 / 6-8
        assert (suffix(7, row * 9, row * 9 + 1) == 2) == (row <= 2)
        assert (suffix(7 | 0x10, row * 9, row * 9 + 1, side=1) == 2) == (row >= 6)


# ------------------------------------------------------------------ known answers
@pytest.mark.parametrize("mode,spatial", MODES)
def test_known_answers_of_the_reference(mode, spatial):
    names = set()
    for v in vectors():
        names.add(v["name"])
        legal = v["legal"] if v["legal"] is not None else [v["move"]]
        row = pack_row([move_action(m, v["side"], spatial) for m in legal], spatial)
        a = move_action(v["move"], v["side"], spatial)
        note = host_move_note(vector_board(v), v["side"], row, a, mode)
        assert hodges_notation(note, mode) == v["hodges"], v["name"]
        assert move_usi(note, spatial) == v["usi"], v["name"]
        d = decode_move_note(note, mode)
        assert d["action"] == a and d["valid"] and d["color"] == ("white" if v["side"] else "black"), v["name"]
    # every case the issue lists is there
    for want in ("simple_move", "capture", "promotion", "declined_promotion", "white_declined_promotion", "promoted_piece_moving",
                 "disambig_file_1", "disambig_rank_2", "three_golds_2", "king_never_disambiguated", "forced_pawn_promote",
                 "forced_pawn_flag_missing", "forced_knight_flag_missing", "forced_lance_flag_missing",
                 "white_forced_pawn_flag_missing", "white_forced_knight_flag_missing", "missing_piece", "corner_king_top_right",
                 "corner_king_bottom_left", "drop_corner", *(f"drop_{l}" for l in "PLNSGBR")):
        assert want in names, want


@pytest.mark.parametrize("mode,spatial", MODES)
def test_vectors_with_kings_hold_in_a_real_position(mode, spatial):
    """What the device test plays: with the kings placed, the oracle calls the move legal and its full legal mask gives
    the same strings as the hand-made list."""
    n = 0
    for v in vectors():
        if v["kings"] is None:
            continue
        n += 1
        board = vector_board(v, kings=True)
        env = so.OracleVecEnv(1, 500, "katago", mode)
        env.set_state(0, board, vector_hands(v), v["side"])
        assert not env.in_check(0, v["side"] ^ 1)
        mask = env.observe(0)[1]
        a = move_action(v["move"], v["side"], spatial)
        assert mask[a], v["name"]
        note = host_move_note(board, v["side"], pack_mask(mask), a, spatial)
        assert (hodges_notation(note, spatial), move_usi(note, spatial)) == (v["hodges"], v["usi"]), v["name"]
    assert n >= 30


def test_full_square_disambiguation():
    """Three black silvers on 41, 57, 59 that all reach 49: the mover on 59 shares its file with 41 and its rank with 57."""
    board = np.zeros(81, np.uint8)
    board[[41, 57, 59]] = 4
    board[72], board[8] = 8, 8 | 0x10
    env = so.OracleVecEnv(1, 500)
    env.set_state(0, board, np.zeros((2, 7), np.uint8), 0)
    mask = env.observe(0)[1]
    to49 = [int(a) for a in np.flatnonzero(mask) if so.decode(int(a), False, True)[1] == 49]
    assert to49 == [5739, 7931, 8257]
    row = pack_mask(mask)
    text = {a: hodges_notation(host_move_note(board, 0, row, a, "spatial"), "spatial") for a in to49}
    assert text[8257] == "S4g-5f"
    assert text[5739] == "Se-5f" and text[7931] == "S6-5f"
    assert decode_move_note(host_move_note(board, 0, row, 8257, 1), 1)["disambiguation"] == 3
    by_name = {v["name"]: v for v in vectors()}
    for a in to49:
        v = by_name[f"three_silvers_black_{a}"]
        assert v["spatial_action"] == a == move_action(v["move"], 0, 1) and v["hodges"] == text[a]
        assert np.array_equal(vector_board(v), board)


def test_actions_the_env_refuses_give_a_bare_note():
    board, _, _ = parse_sfen(START)
    row = np.full((G.DEFAULT_ACTION_SPACE + 31) // 32, 0xFFFFFFFF, np.uint32)
    for mode, A in ((1, G.ACTION_SPACE), (0, G.DEFAULT_ACTION_SPACE)):
        for a in (-1, A, A + 7, 1 << 31, -(1 << 40)):
            assert host_move_note(board, 0, row, a, mode) == 0
    assert host_move_note(board, 0, row, 0, 1) == 0            # square 0, one step north: off the board
    off = 80 * 139 + 4 * 8                                     # square 80, one step south
    assert host_move_note(board, 0, row, off, 1) == off
    assert not decode_move_note(off, 1)["valid"] and hodges_notation(off, 1) == "?" and move_usi(off, 1) == "?"


# ------------------------------------------------------------------ an independent restatement over playouts
_LETTER = {v: k for k, v in TYPES.items()}


def _sq(s: int) -> str:
    return f"{9 - s % 9}{chr(ord('a') + s // 9)}"


def reference_strings(board, side: int, mask: np.ndarray, action: int, spatial: int):
    """move_notation / move_usi (spectator_data.rs:93-186) from the decoded legal move list, as the reference builds them."""
    frm, to, promote, drop = so.decode(int(action), bool(side), bool(spatial))
    if drop:
        return f"{_LETTER[drop]}*{_sq(to)}", f"{_LETTER[drop]}*{_sq(to)}"
    usi = _sq(frm) + _sq(to) + ("+" if promote else "")
    piece = int(board[frm])
    if not piece:
        return f"?{_sq(frm)}-{_sq(to)}", usi
    pt, white, promoted = piece & 15, bool(piece & 0x10), bool(piece & 0x20)
    dis = ""
    if pt != 8:
        others = []
        for other in np.flatnonzero(mask):
            of, ot, _, od = so.decode(int(other), bool(side), bool(spatial))
            if od or ot != to or of == frm or not board[of]:
                continue
            if (int(board[of]) & 15) == pt and bool(int(board[of]) & 0x20) == promoted:
                others.append(of)
        if others:
            if not any(o % 9 == frm % 9 for o in others):
                dis = str(9 - frm % 9)
            elif not any(o // 9 == frm // 9 for o in others):
                dis = chr(ord("a") + frm // 9)
            else:
                dis = _sq(frm)
    row = to // 9
    forced = (pt in (1, 2) and row == (8 if white else 0)) or (pt == 3 and (row >= 7 if white else row <= 1))
    zone = lambda s: (s // 9 >= 6) if white else (s // 9 <= 2)  # noqa: E731
    if promote or forced:
        suffix = "+"
    elif pt in (1, 2, 3, 4, 6, 7) and not promoted and (zone(frm) or zone(to)):
        suffix = "="
    else:
        suffix = ""
    return f"{'+' if promoted else ''}{_LETTER[pt]}{dis}{'x' if board[to] else '-'}{_sq(to)}{suffix}", usi


@pytest.mark.parametrize("mode,spatial", MODES)
def test_host_note_against_the_restated_reference_over_playouts(mode, spatial):
    games, plies = 8, 150
    env = so.OracleVecEnv(games, 500, "katago", mode)
    _, mask = env.reset()
    rng = np.random.default_rng(PLAY_SEED)
    seen = dict(capture=0, drop=0, plus=0, equals=0, promoted=0, disambiguated=0)
    for _ in range(plies):
        acts = np.array([rng.choice(np.flatnonzero(m)) for m in mask], np.int64)
        for e in range(games):
            board, _, side, _ = env.state(e)
            want = reference_strings(board, side, mask[e], int(acts[e]), spatial)
            note = host_move_note(board, side, pack_mask(mask[e]), int(acts[e]), mode)
            assert (hodges_notation(note, mode), move_usi(note, mode)) == want, (e, int(acts[e]))
            text = want[0]
            seen["capture"] += "x" in text
            seen["drop"] += "*" in text
            seen["plus"] += text.endswith("+")
            seen["equals"] += text.endswith("=")
            seen["promoted"] += text.startswith("+")
            seen["disambiguated"] += re.match(r"^\+?[A-Z][1-9a-i]{1,2}[-x]", text) is not None
        mask = env.step(acts)["legal_masks"]
    assert all(seen.values()), seen


# ------------------------------------------------------------------ the dict builder (reference: test_vec_env.py:8-66, 114-120)
def start_rows(n: int) -> np.ndarray:
    board, hands, side = parse_sfen(START)
    rows = np.zeros((n, 128), np.uint8)
    rows[:, :81], rows[:, 81:95], rows[:, 95] = board, hands.reshape(14), side
    return rows


def test_spectator_dicts_list_and_keys():
    data = spectator_dicts(start_rows(3))
    assert isinstance(data, list) and len(data) == 3
    assert set(data[0].keys()) == {"board", "hands", "current_player", "ply", "is_over", "result", "sfen", "in_check",
                                   "move_history"}


def test_spectator_dicts_startpos_values():
    d = spectator_dicts(start_rows(1))[0]
    assert d["current_player"] == "black" and d["ply"] == 0
    assert d["is_over"] is False and d["result"] == "in_progress" and d["in_check"] is False
    assert len(d["board"]) == 81 and "lnsgkgsnl" in d["sfen"].lower()
    assert d["move_history"] == []
    assert d["board"][0] == {"type": "lance", "color": "white", "promoted": False, "row": 0, "col": 0}
    assert d["board"][76] == {"type": "king", "color": "black", "promoted": False, "row": 8, "col": 4}
    assert d["board"][40] is None and sum(p is not None for p in d["board"]) == 40
    assert all(type(p["row"]) is int and type(p["promoted"]) is bool for p in d["board"] if p)


def test_spectator_dicts_hands_structure():
    rows = start_rows(1)
    rows[0, 81:95] = np.arange(14)
    d = spectator_dicts(rows)[0]
    order = ["pawn", "lance", "knight", "silver", "gold", "bishop", "rook"]
    assert list(d["hands"]) == ["black", "white"] and list(d["hands"]["black"]) == order == list(d["hands"]["white"])
    assert [d["hands"]["black"][k] for k in order] == list(range(7))
    assert [d["hands"]["white"][k] for k in order] == list(range(7, 14))
    assert spectator_dicts(start_rows(1))[0]["hands"]["black"]["pawn"] == 0


def test_spectator_dicts_follow_the_state_row():
    env = so.OracleVecEnv(2, 100)
    _, mask = env.reset()
    env.step(np.array([np.flatnonzero(mask[0])[0], np.flatnonzero(mask[1])[-1]], np.int64))
    rows = np.zeros((2, 128), np.uint8)
    for e in range(2):
        board, hands, side, ply = env.state(e)
        rows[e, :81], rows[e, 81:95], rows[e, 95], rows[e, 96] = board, hands.reshape(14), side, e
        rows[e, 100:104] = np.frombuffer(np.uint32(ply).tobytes(), np.uint8)
    data = spectator_dicts(rows)
    for e, d in enumerate(data):
        board, hands, side, _ = env.state(e)
        assert d["ply"] == 1 and d["current_player"] == "white" and d["in_check"] is bool(e)
        assert d["sfen"] == format_sfen(board, hands, side)
    assert data[0]["sfen"] != data[1]["sfen"]


def test_spectator_dicts_histories_and_the_snapshot_rows_serialise():
    v = next(x for x in vectors() if x["name"] == "capture")
    a = move_action(v["move"], 0, 1)
    note = host_move_note(vector_board(v), 0, pack_row([a], 1), a, 1)
    data = spectator_dicts(start_rows(2), [[note], []], "spatial")
    assert data[0]["move_history"] == [{"action": a, "notation": "Bx3c=", "usi": "8h3c"}] and data[1]["move_history"] == []
    rows = [{"game_id": i, "board_json": json.dumps(d.get("board", [])), "hands_json": json.dumps(d.get("hands", {})),
             "current_player": d.get("current_player", "black"), "ply": d.get("ply", 0), "is_over": int(d.get("is_over", False)),
             "result": d.get("result", "in_progress"), "sfen": d.get("sfen", ""), "in_check": int(d.get("in_check", False)),
             "move_history_json": json.dumps(d.get("move_history", []))} for i, d in enumerate(data)]     # katago_loop.py:1924-1948
    assert json.loads(json.dumps(rows))[0]["ply"] == 0 and json.loads(rows[0]["move_history_json"])[0]["usi"] == "8h3c"
