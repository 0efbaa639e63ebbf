"""Game record parsers for supervised learning (API mirror of keisei/sl/parsers.py).

Two text formats, each yielding ``GameRecord``s with USI moves:

``.sfen``  blocks separated by a blank line: ``key:value`` metadata lines (``result:win_black|win_white|draw`` is
           required), one position line (``startpos`` or an SFEN), then one USI move per line.
``.csa``   CSA V2.2 as Floodgate writes it; games of one archive are separated by a ``/`` line.  Moves become USI; a
           promotion is a promoted piece name arriving from a square that held an unpromoted piece.

One field is added to the reference's record: ``GameRecord.start`` keeps where the game starts -- the position line of an
SFEN block, ``"startpos"`` for a CSA game on the standard board -- because the device replay (keisei_amd.sl.prepare) starts
every game from the standard position and has to leave other games out.
"""
from __future__ import annotations

import logging
from abc import ABC, abstractmethod
from dataclasses import dataclass, field
from enum import Enum
from pathlib import Path
from typing import Dict, Iterator, List, Optional, Set, Tuple

logger = logging.getLogger(__name__)

STARTPOS = "startpos"
START_SFEN = "lnsgkgsnl/1r5b1/ppppppppp/9/9/9/PPPPPPPPP/1B5R1/LNSGKGSNL b - 1"


class GameOutcome(Enum):
    WIN_BLACK = "win_black"
    WIN_WHITE = "win_white"
    DRAW = "draw"


@dataclass
class ParsedMove:
    move_usi: str
    sfen_before: str = ""


@dataclass
class GameRecord:
    moves: List[ParsedMove]
    outcome: GameOutcome
    metadata: Dict[str, str] = field(default_factory=dict)
    start: str = STARTPOS


@dataclass
class GameFilter:
    """Quality gate in front of the encoder: a minimum length, and a minimum for every rating the record states."""

    min_ply: int = 40
    min_rating: Optional[int] = None

    def accepts(self, record: GameRecord) -> bool:
        if len(record.moves) < self.min_ply:
            return False
        if self.min_rating is None:
            return True
        stated = (record.metadata.get(k, "") for k in ("rating", "black_rating", "white_rating"))
        return not any(s.isdigit() and int(s) < self.min_rating for s in stated)


class GameParser(ABC):
    @abstractmethod
    def parse(self, path: Path) -> Iterator[GameRecord]: ...

    @abstractmethod
    def supported_extensions(self) -> Set[str]: ...


def _unix_newlines(text: str) -> str:
    return text.replace("\r\n", "\n").replace("\r", "\n")


def is_standard_start(start: str) -> bool:
    """``startpos`` or the standard position written out as an SFEN (the move counter is not compared)."""
    s = start.strip()
    if s.startswith("sfen "):
        s = s[5:].strip()
    if s.startswith("position "):
        s = s[9:].strip()
    if s == STARTPOS:
        return True
    return s.split()[:3] == START_SFEN.split()[:3]


class SFENParser(GameParser):
    def supported_extensions(self) -> Set[str]:
        return {".sfen"}

    @staticmethod
    def _is_metadata(line: str) -> bool:
        # "key:value" with no digit in the key (a digit there would be a move or an SFEN field)
        key, colon, _ = line.partition(":")
        return bool(colon) and not any(ch.isdigit() for ch in key)

    def parse(self, path: Path) -> Iterator[GameRecord]:
        for block in _unix_newlines(path.read_text()).strip().split("\n\n"):
            lines = [ln.strip() for ln in block.strip().split("\n")]
            lines = [ln for ln in lines if ln]
            if len(lines) < 2:
                continue
            metadata: Dict[str, str] = {}
            at = 0
            while at < len(lines) and self._is_metadata(lines[at]):
                key, _, value = lines[at].partition(":")
                metadata[key.strip()] = value.strip()
                at += 1
            try:
                outcome = GameOutcome(metadata.get("result", ""))
            except ValueError:
                continue                                        # a game without a known result teaches the value head nothing
            start = STARTPOS
            if at < len(lines):                                 # the position line
                start = lines[at]
                at += 1
            moves = [ParsedMove(move_usi=ln) for ln in lines[at:]]
            if moves:
                yield GameRecord(moves=moves, outcome=outcome, metadata=metadata, start=start)


_RANKS = "abcdefghi"
_CSA_TO_USI = {"FU": "P", "KY": "L", "KE": "N", "GI": "S", "KI": "G", "KA": "B", "HI": "R", "OU": "K",
               "TO": "P", "NY": "L", "NK": "N", "NG": "S", "UM": "B", "RY": "R"}
_CSA_PROMOTED = frozenset(("TO", "NY", "NK", "NG", "UM", "RY"))
_BACK_RANK = ("KY", "KE", "GI", "KI", "OU", "KI", "GI", "KE", "KY")      # files 9..1
_LAST_MOVER_WINS = frozenset(("%TORYO", "%TIME_UP", "%ILLEGAL_MOVE", "%JISHOGI", "%KACHI"))
_DRAWS = frozenset(("%SENNICHITE", "%HIKIWAKE"))
Board = Dict[Tuple[int, int], str]                                       # (file, rank) -> CSA piece name, colour not kept


def _rank(row: int) -> str:
    if not 1 <= row <= 9:
        raise KeyError(row)                                     # the block is skipped (CSAParser.parse)
    return _RANKS[row - 1]


def _standard_board() -> Board:
    board: Board = {}
    for k, name in enumerate(_BACK_RANK):
        board[(9 - k, 1)] = name
        board[(9 - k, 9)] = name
    for f in range(1, 10):
        board[(f, 3)] = "FU"
        board[(f, 7)] = "FU"
    board[(8, 2)], board[(2, 2)] = "HI", "KA"
    board[(8, 8)], board[(2, 8)] = "KA", "HI"
    return board


def _coloured_standard_board() -> Dict[Tuple[int, int], str]:
    return {sq: ("-" if sq[1] <= 3 else "+") + name for sq, name in _standard_board().items()}


class CSAParser(GameParser):
    def supported_extensions(self) -> Set[str]:
        return {".csa"}

    # ------------------------------------------------------------------ position
    @staticmethod
    def _cells(p_lines: List[str]) -> Dict[Tuple[int, int], str]:
        """P1..P9 lines -> (file, rank) -> the 3-character cell with its colour sign."""
        cells: Dict[Tuple[int, int], str] = {}
        for line in p_lines:
            if len(line) < 3 or line[0] != "P" or not line[1].isdigit():
                continue
            rank, body = int(line[1]), line[2:]
            for k in range(9):
                cell = body[3 * k:3 * k + 3]
                if len(cell) < 3:
                    break
                if cell.strip() in ("*", ""):
                    continue
                cells[(9 - k, rank)] = cell
        return cells

    @classmethod
    def _parse_board_from_p_lines(cls, p_lines: List[str]) -> Board:
        return {sq: cell[1:3] for sq, cell in cls._cells(p_lines).items()}

    @classmethod
    def _init_board(cls, p_lines: List[str], pi_line: Optional[str], pp_lines: List[str]) -> Board:
        if p_lines:
            board = cls._parse_board_from_p_lines(p_lines)
        elif pi_line is not None:
            board = _standard_board()
            removed = pi_line[2:]                               # "PI82HI22KA": squares left empty (handicaps)
            for k in range(0, len(removed) - 3, 4):
                board.pop((int(removed[k]), int(removed[k + 1])), None)
        else:
            board = {}
        for line in pp_lines:                                   # "P+63FU00KI": single placements; 00 = in hand
            body = line[2:]
            for k in range(0, len(body) - 3, 4):
                f, r = int(body[k]), int(body[k + 1])
                if (f, r) != (0, 0):
                    board[(f, r)] = body[k + 2:k + 4]
        return board

    @classmethod
    def _start_of(cls, p_lines: List[str], pi_line: Optional[str], pp_lines: List[str], first_side: str) -> str:
        """``"startpos"`` for the standard board with black to move; a short description of what differs otherwise."""
        if pp_lines:
            return "csa:placements"
        if first_side == "-":
            return "csa:white_to_move"
        if p_lines:
            return STARTPOS if cls._cells(p_lines) == _coloured_standard_board() else "csa:board"
        if pi_line is not None:
            return STARTPOS if pi_line == "PI" else "csa:" + pi_line
        return "csa:no_position"

    # ------------------------------------------------------------------ moves
    def _csa_move_to_usi(self, csa_move: str, board: Board) -> str:
        """``+7776FU`` -> ``7g7f``; ``-0055KA`` -> ``B*5e``.  The piece name is the piece AFTER the move."""
        body = csa_move[1:]
        ff, fr, tf, tr = (int(ch) for ch in body[:4])
        piece = body[4:]
        to = f"{tf}{_rank(tr)}"
        if (ff, fr) == (0, 0):
            return f"{_CSA_TO_USI.get(piece, piece)}*{to}"
        promotes = piece in _CSA_PROMOTED and board.get((ff, fr), "") not in _CSA_PROMOTED
        return f"{ff}{_rank(fr)}{to}" + ("+" if promotes else "")

    # ------------------------------------------------------------------ files
    @staticmethod
    def _read(path: Path) -> str:
        try:
            return path.read_text(encoding="utf-8")
        except UnicodeDecodeError:
            pass
        try:
            import chardet
        except ImportError:
            logger.warning("Non-UTF-8 file %s decoded as Shift-JIS (chardet not available)", path.name)
            return path.read_text(encoding="shift_jis", errors="replace")
        raw = path.read_bytes()
        guess = chardet.detect(raw)
        encoding = guess.get("encoding", "shift_jis") or "shift_jis"
        logger.info("Decoded %s as %s (confidence %.0f%%)", path.name, encoding, (guess.get("confidence", 0) or 0) * 100)
        return raw.decode(encoding, errors="replace")

    def parse(self, path: Path) -> Iterator[GameRecord]:
        for n, block in enumerate(_unix_newlines(self._read(path)).split("\n/\n")):
            block = block.strip()
            if not block:
                continue
            try:
                record = self._parse_single_game(block)
            except Exception:
                logger.exception("Failed to parse CSA game block %d in %s — skipping", n, path.name)
                continue
            if record is not None:
                yield record

    def _parse_single_game(self, text: str) -> Optional[GameRecord]:
        lines = [ln.strip() for ln in text.split("\n")]
        p_lines = [ln for ln in lines if len(ln) >= 2 and ln[0] == "P" and ln[1].isdigit()]
        pi_lines = [ln for ln in lines if len(ln) >= 2 and ln[:2] == "PI"]
        pp_lines = [ln for ln in lines if len(ln) >= 2 and ln[:2] in ("P+", "P-")]
        pi_line = pi_lines[-1] if pi_lines else None
        board = self._init_board(p_lines, pi_line, pp_lines)

        metadata: Dict[str, str] = {}
        moves: List[ParsedMove] = []
        last_mover, result, first_side = "+", "", ""
        for line in lines:
            if not line or line[0] in ("'", "V", "P"):          # blank, comment, version, position (read above)
                continue
            if line[:2] in ("N+", "N-"):
                metadata["player_black" if line[1] == "+" else "player_white"] = line[2:]
            elif line[0] == "$":
                key, _, value = line[1:].partition(":")
                metadata[key.lower()] = value.strip()
            elif line in ("+", "-"):                            # side to move
                first_side = first_side or line
            elif line[0] == "%":
                result = line
            elif line[0] in "+-":
                if "%" in line:                                 # "+%TORYO": the resigning side writes it, the mover stays
                    result = line[1:]
                    continue
                body = line[1:]
                if len(body) < 5:
                    logger.warning("Skipping malformed CSA move (too short): %r", line)
                    return None
                last_mover = line[0]
                moves.append(ParsedMove(move_usi=self._csa_move_to_usi(line, board)))
                src, dst = (int(body[0]), int(body[1])), (int(body[2]), int(body[3]))
                if src != (0, 0):
                    board.pop(src, None)
                board[dst] = body[4:]
        if not moves:
            return None
        if result in _LAST_MOVER_WINS:                          # the side to move resigned, lost on time, ... or the mover declared
            outcome = GameOutcome.WIN_BLACK if last_mover == "+" else GameOutcome.WIN_WHITE
        elif result in _DRAWS:
            outcome = GameOutcome.DRAW
        elif result == "%CHUDAN":                               # interrupted: no result
            return None
        else:
            logger.warning("Unknown CSA result '%s', skipping game", result)
            return None
        return GameRecord(moves=moves, outcome=outcome, metadata=metadata,
                          start=self._start_of(p_lines, pi_line, pp_lines, first_side))
