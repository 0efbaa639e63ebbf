"""GameLog: the moves of the games played on the device (the reference's per-env ``move_history``, vec_env.rs:259, cleared
on auto-reset, and the move lists it stores with showcase games).

The loops that play on the device never hand a move to the host, so a game can only be kept by a kernel inside the ply.
``GameLog`` owns the buffers of csrc/gamelog.hip (include/keisei_amd.h, "game log"): per env a move row, a start slot and
four meta words; a store of ``capacity`` finished games; a four-word cursor.  One launch per ply (``step``, or ``step_env``
where the players are per env, as in the league rollout), no host synchronisation, capturable in the rollout graphs;
``drain()`` at the owner's sync point reads the cursor, copies exactly the committed records and zeroes the cursor;
``live()`` at a sync point hands out the games still in progress (the reference's ``move_history`` can be read at any time).

Three uses of a drained ``RecordedGame``: ``write_sfen_games`` writes ``.sfen`` files this package's ``SFENParser`` reads
back; ``keisei_amd.sl.prepare.dataset_from_recorded_games`` builds a ``DeviceSLDataset`` from them; ``actions`` and the
start position replay on the CPU oracle.

``HostGameLog`` restates the kernels in numpy over the same buffers, word for word; ``game_log_host`` runs a whole
script of plies through it.  The tests hold the kernels to it.
"""
from __future__ import annotations

from dataclasses import dataclass
from pathlib import Path
from typing import Dict, Iterable, List, Mapping, Optional, Sequence, Union

import numpy as np
import torch

from keisei_amd import _lib
from keisei_amd.shogi_gym import POOL_ROW_BYTES, SpatialActionMapper, format_sfen

__all__ = ["GameLog", "RecordedGame", "HostGameLog", "game_log_host", "games_from_records", "usi_of", "write_sfen_games"]

# layout of csrc/gamelog.hip
HEAD_WORDS, START_WORDS, CURSOR_WORDS, META_WORDS = 12, POOL_ROW_BYTES // 4, 4, 4
TRUNCATED_ONLY, CARRIED = 1, 2                                   # flag bits of a record
_ENV, _PLIES, _WINNER, _REASON, _FLAGS, _BLACK, _WHITE, _END_PLY, _GAME, _LEARNER = range(10)
_HAND = "PLNSGBR"
_MAPPER = SpatialActionMapper()
_RESULT = ("win_black", "win_white", "draw")
_START_BOARD = None


def record_words(max_ply: int) -> int:
    """int32 words of one game record: header, start position, ``max_ply`` moves two per word."""
    return HEAD_WORDS + START_WORDS + (int(max_ply) + 1) // 2


def _square_usi(sq: int) -> str:
    """Row-major square of ``VecEnv.get_sfen`` (row 0 is rank 'a', column 0 is file 9) in USI."""
    return f"{9 - sq % 9}{'abcdefghi'[sq // 9]}"


def usi_of(action: int, is_white: bool) -> str:
    """The USI text of a spatial action index for the side that plays it: the inverse of
    ``keisei_amd.sl.prepare.usi_to_action``.  Raises ``ValueError`` where ``SpatialActionMapper.decode`` does."""
    m = _MAPPER.decode(int(action), bool(is_white))
    if m["type"] == "drop":
        return f"{_HAND[m['piece_type_idx']]}*{_square_usi(m['to_sq'])}"
    return _square_usi(m["from_sq"]) + _square_usi(m["to_sq"]) + ("+" if m["promote"] else "")


def _standard_start_row() -> np.ndarray:
    global _START_BOARD
    if _START_BOARD is None:
        from keisei_amd.shogi_gym import parse_sfen
        from keisei_amd.sl.parsers import START_SFEN

        board, hands, side = parse_sfen(START_SFEN)
        _START_BOARD = np.concatenate([np.asarray(board, np.uint8).reshape(81), np.asarray(hands, np.uint8).reshape(14),
                                       np.asarray([side], np.uint8)])
    return _START_BOARD


@dataclass
class RecordedGame:
    """One game as the device logged it: finished (a drained record) or still in progress (a peeked row)."""
    start_board: np.ndarray             # uint8 (81,), the piece bytes of the env's state row
    start_hands: np.ndarray             # uint8 (2, 7)
    start_side: int                     # the side to move at the start: 0 black, 1 white
    actions: np.ndarray                 # uint16 (plies,), spatial action indices in the mover's perspective
    winner: int                         # 0 black, 1 white, 2 draw; -1 for a game in progress
    reason: int                         # the env's TerminationReason of the last ply
    truncated: bool                     # cut at max_ply, not decided
    carried: bool                       # a ply of it was not played by the pairing named here (idle or inherited)
    env: int
    black: int                          # -1 where the owner names no players (self-play)
    white: int
    end_ply: int                        # the owner's ply counter at the game's last ply
    game_number: int                    # games the env had finished before this one, since begin()
    finished: bool = True               # False: a game in progress as ``live()`` peeked it (winner -1, end_ply = now)
    learner_side: Optional[int] = None  # 0 black, 1 white where the owner has a learner (the league rollout), else None

    def start_sfen(self) -> str:
        return format_sfen(self.start_board, self.start_hands, int(self.start_side))

    @property
    def is_standard_start(self) -> bool:
        row = _standard_start_row()
        return bool(np.array_equal(self.start_board, row[:81]) and np.array_equal(self.start_hands.reshape(14), row[81:95])
                    and int(self.start_side) == int(row[95]))

    def usi_moves(self) -> List[str]:
        return [usi_of(int(a), bool((int(self.start_side) + i) & 1)) for i, a in enumerate(self.actions)]

    @property
    def outcome(self):
        from keisei_amd.sl.parsers import GameOutcome

        if not self.finished:
            raise ValueError(f"the game in progress in env {self.env} has no outcome yet")
        return (GameOutcome.WIN_BLACK, GameOutcome.WIN_WHITE, GameOutcome.DRAW)[int(self.winner)]

    @property
    def learner_result(self) -> Optional[str]:
        """``"win"`` / ``"loss"`` / ``"draw"`` in the learner's frame; None without a learner or for a game in progress."""
        if self.learner_side is None or not self.finished:
            return None
        if int(self.winner) == 2:
            return "draw"
        return "win" if int(self.winner) == int(self.learner_side) else "loss"


def games_from_records(records: np.ndarray) -> List[RecordedGame]:
    """Decode records (int32 rows of ``record_words(max_ply)`` words) into games, in their order.  A row with winner -1
    is a game in progress (``ka_gamelog_peek``); header word 9 is the learner's colour + 1, 0 where there is no learner."""
    out = []
    records = np.ascontiguousarray(records, dtype=np.int32)
    for rec in records:
        n = int(rec[_PLIES])
        start = rec[HEAD_WORDS:HEAD_WORDS + START_WORDS].copy().view(np.uint8)
        moves = rec[HEAD_WORDS + START_WORDS:].copy().view(np.uint16)[:n].copy()
        flags = int(rec[_FLAGS])
        out.append(RecordedGame(start[:81].copy(), start[81:95].reshape(2, 7).copy(), int(start[95]), moves,
                                int(rec[_WINNER]), int(rec[_REASON]), bool(flags & TRUNCATED_ONLY), bool(flags & CARRIED),
                                int(rec[_ENV]), int(rec[_BLACK]), int(rec[_WHITE]), int(rec[_END_PLY]), int(rec[_GAME]),
                                int(rec[_WINNER]) >= 0, int(rec[_LEARNER]) - 1 if int(rec[_LEARNER]) in (1, 2) else None))
    return out


def write_sfen_games(path, games: Iterable[RecordedGame], *,
                     metadata: Union[None, Mapping[str, str], Sequence[Mapping[str, str]]] = None) -> int:
    """Write ``games`` as one ``.sfen`` file in the shape ``SFENParser.parse`` reads: per game a ``result:`` line, the
    ``key:value`` metadata lines (``black``, ``white`` when the game names its players, ``reason``, and ``metadata`` --
    one mapping for every game or one per game; a key may hold no digit and no colon), the position line (``startpos`` or
    the SFEN), one USI move per line; a blank line between games.  A game without a move is not written (the parser
    would drop the block).  A game in progress raises ``ValueError``: the format needs a result.  Returns the number of
    games written."""
    games = list(games)
    for g in games:
        if not g.finished:
            raise ValueError(f"the game in progress in env {g.env} (game {g.game_number}) has no result yet: a .sfen block "
                             "needs one; write finished games")
    if metadata is not None and not isinstance(metadata, Mapping):
        metadata = list(metadata)
        if len(metadata) != len(games):
            raise ValueError(f"metadata names {len(metadata)} games, there are {len(games)}")
    blocks = []
    for i, g in enumerate(games):
        if len(g.actions) == 0:
            continue
        meta: Dict[str, str] = {}
        if g.black >= 0 or g.white >= 0:
            meta["black"], meta["white"] = str(g.black), str(g.white)
        meta["reason"] = str(g.reason)
        extra = metadata if isinstance(metadata, Mapping) or metadata is None else metadata[i]
        for k, v in (extra or {}).items():
            k, v = str(k), str(v)
            if not k.strip() or ":" in k or any(ch.isdigit() for ch in k) or k.strip() == "result":
                raise ValueError(f"metadata key {k!r}: a key is not empty, not 'result', and holds no digit and no colon")
            if "\n" in v or "\r" in v:
                raise ValueError(f"metadata value of {k!r} spans lines")
            meta[k.strip()] = v.strip()
        lines = [f"result:{_RESULT[int(g.winner)]}"] + [f"{k}:{v}" for k, v in meta.items()]
        lines.append("startpos" if g.is_standard_start else g.start_sfen())
        lines += g.usi_moves()
        blocks.append("\n".join(lines))
    Path(path).write_text("\n\n".join(blocks) + ("\n" if blocks else ""))
    return len(blocks)


# ---------------------------------------------------------------------------------------------- host restatement
class HostGameLog:
    """``ka_gamelog_begin`` / ``ka_gamelog_step`` / ``ka_gamelog_step_env`` / ``ka_gamelog_peek`` / ``ka_gamelog_seat``
    in numpy, over buffers of the device's layout:
    ``rows`` uint16 (E, row_stride), ``meta`` int32 (E, 4), ``starts`` int32 (E, 24), ``records`` int32 (capacity,
    record_words(max_ply)), ``cursor`` int32 (4,).  Words the kernel does not write keep what they held."""

    def __init__(self, num_envs: int, max_ply: int, capacity: int, *, row_stride: Optional[int] = None, fill: int = 0) -> None:
        self.num_envs, self.max_ply, self.capacity = int(num_envs), int(max_ply), int(capacity)
        self.row_stride = 2 * ((self.max_ply + 1) // 2) if row_stride is None else int(row_stride)
        if self.row_stride % 2 or self.row_stride < self.max_ply:
            raise ValueError(f"row_stride must be even and at least max_ply, got {self.row_stride}")
        E = self.num_envs
        self.rows = np.full((E, self.row_stride), fill & 0xFFFF, np.uint16)
        self.meta = np.zeros((E, META_WORDS), np.int32)
        self.starts = np.zeros((E, START_WORDS), np.int32)
        self.records = np.full((self.capacity, record_words(self.max_ply)), fill, np.int32)
        self.cursor = np.zeros(CURSOR_WORDS, np.int32)

    @staticmethod
    def _start_words(state_rows) -> np.ndarray:
        s = np.ascontiguousarray(np.asarray(state_rows, np.uint8)[:, :POOL_ROW_BYTES])
        return s.view(np.int32).reshape(-1, START_WORDS)

    def begin(self, state_rows) -> None:
        self.meta[:] = 0
        self.starts[:] = self._start_words(state_rows)

    def seat(self, jobs, slots: int, envs_per_slot: int) -> None:
        for job in np.asarray(jobs).reshape(-1, 4):
            s = int(job[0])
            if 0 <= s < slots:
                m = self.meta[s * envs_per_slot:(s + 1) * envs_per_slot]
                m[m[:, 0] > 0, 1] = 1

    def step(self, state_rows, actions, rewards, terminated, truncated, pre_player, reason, *, nlegal=None, live=None,
             pairs=None, pair_stride: int = 0, envs_per_pair: int = 1, ply_counter: int = 0, side=None, opp=None,
             ids=None) -> None:
        """One ply; ``state_rows`` is the env state AFTER the env step (finished games already restarted).  With ``side``
        / ``opp`` / ``ids`` (the per-env players) it is ``ka_gamelog_step_env``, else ``ka_gamelog_step``."""
        E = self.num_envs
        per_env = side is not None or opp is not None or ids is not None
        if per_env and pairs is not None:
            raise ValueError("the players come from pairs or from side / opp / ids, not both")
        if per_env and (side is None or opp is None or ids is None):
            raise ValueError("per-env players need side, opp and ids together")
        starts_now = self._start_words(state_rows)
        tm, tr = np.asarray(terminated).astype(bool), np.asarray(truncated).astype(bool)
        rewards = np.asarray(rewards, np.float32)
        G = int(envs_per_pair) if pairs is not None else 1
        stalled = np.zeros((E + G - 1) // G, bool)
        if nlegal is not None:
            for e in np.flatnonzero(np.asarray(nlegal) == 0):
                stalled[e // G] = True
        first = int(self.cursor[0])
        room = 0 if first < 0 else max(0, self.capacity - first)
        rank = 0
        for e in range(E):
            count = int(self.meta[e, 0])
            if count < self.max_ply:
                self.rows[e, count] = np.uint16(int(actions[e]) & 0xFFFF)
            plies = min(count + 1, self.max_ply)
            is_live = True if live is None else int(live[e]) >= 0
            carried = (int(self.meta[e, 1]) | (0 if is_live else 1)) & 1
            done = bool(tm[e] or tr[e])
            if per_env:
                s, tag = int(side[e]) & 1, _player_tag(side[e], opp[e])
                if count > 0 and int(self.meta[e, 3]) != tag:
                    carried = 1
            if done and is_live and not stalled[e // G]:
                if rank < room:
                    rec = self.records[first + rank]
                    r, pre = rewards[e], int(pre_player[e]) & 1
                    black = white = -1
                    if pairs is not None:
                        p = np.asarray(pairs).reshape(-1)[(e // G) * pair_stride:]
                        black, white = int(p[0]), int(p[1])
                    if per_env:
                        black, white = _env_players(ids, s, opp[e])
                    rec[:HEAD_WORDS] = [e, plies, pre if r > 0 else (1 - pre if r < 0 else 2), int(reason[e]),
                                        (TRUNCATED_ONLY if tr[e] and not tm[e] else 0) | (CARRIED if carried else 0),
                                        black, white, int(ply_counter), int(self.meta[e, 2]), s + 1 if per_env else 0, 0, 0]
                    rec[HEAD_WORDS:HEAD_WORDS + START_WORDS] = self.starts[e]
                    words = (plies + 1) // 2
                    mv = np.zeros(2 * words, np.uint16)
                    mv[:plies] = self.rows[e, :plies]
                    rec[HEAD_WORDS + START_WORDS:HEAD_WORDS + START_WORDS + words] = mv.view(np.int32)
                rank += 1
            if done:
                self.meta[e, :3] = [0, 0, int(self.meta[e, 2]) + 1]
                self.starts[e] = starts_now[e]
            else:
                self.meta[e, 0], self.meta[e, 1] = plies, carried
            if per_env:
                self.meta[e, 3] = 0 if done else tag
        self.cursor[0] = first + min(rank, room)
        self.cursor[1] += max(0, rank - room)
        self.cursor[2] += 1

    def peek(self, envs=None, *, pairs=None, pair_stride: int = 0, envs_per_pair: int = 1, side=None, opp=None, ids=None,
             ply_counter: int = 0, out: Optional[np.ndarray] = None) -> np.ndarray:
        """``ka_gamelog_peek``: the games in progress of ``envs`` (default: every env) as record-shaped rows, written into
        ``out`` (n, record_words(max_ply)) int32 where given -- words the kernel does not write keep what they held."""
        per_env = side is not None or opp is not None or ids is not None
        if per_env and pairs is not None:
            raise ValueError("the players come from pairs or from side / opp / ids, not both")
        if per_env and (side is None or opp is None or ids is None):
            raise ValueError("per-env players need side, opp and ids together")
        envs = np.arange(self.num_envs) if envs is None else np.asarray(envs, np.int64).reshape(-1)
        if out is None:
            out = np.zeros((len(envs), record_words(self.max_ply)), np.int32)
        G = int(envs_per_pair) if pairs is not None else 1
        for j, e in enumerate(int(v) for v in envs):
            rec = out[j]
            if not 0 <= e < self.num_envs:
                rec[:HEAD_WORDS] = [-1, 0, -1, 0, 0, -1, -1, int(ply_counter), 0, 0, 0, 0]
                rec[HEAD_WORDS:HEAD_WORDS + START_WORDS] = 0
                continue
            n = max(0, min(int(self.meta[e, 0]), self.max_ply))
            black = white = -1
            colour = 0
            if pairs is not None:
                p = np.asarray(pairs).reshape(-1)[(e // G) * pair_stride:]
                black, white = int(p[0]), int(p[1])
            elif per_env:
                s = int(side[e]) & 1
                black, white = _env_players(ids, s, opp[e])
                colour = s + 1
            rec[:HEAD_WORDS] = [e, n, -1, 0, CARRIED if int(self.meta[e, 1]) & 1 else 0, black, white, int(ply_counter),
                                int(self.meta[e, 2]), colour, 0, 0]
            rec[HEAD_WORDS:HEAD_WORDS + START_WORDS] = self.starts[e]
            words = (n + 1) // 2
            mv = np.zeros(2 * words, np.uint16)
            mv[:n] = self.rows[e, :n]
            rec[HEAD_WORDS + START_WORDS:HEAD_WORDS + START_WORDS + words] = mv.view(np.int32)
        return out

    def games(self) -> List[RecordedGame]:
        return games_from_records(self.records[:int(self.cursor[0])])


def _player_tag(side, opp) -> int:
    """((opp << 1) | side) + 1 in the kernel's 32-bit wrapping arithmetic, as an int32 value."""
    t = ((((int(opp) & 0xFFFFFFFF) << 1) & 0xFFFFFFFF) | (int(side) & 1)) + 1 & 0xFFFFFFFF
    return t - (1 << 32) if t >= 1 << 31 else t


def _env_players(ids, s: int, opp):
    """(black, white) of an env whose learner plays colour ``s`` against opponent index ``opp``: ids[0] is the learner."""
    ids = np.asarray(ids).reshape(-1)
    k = int(opp)
    oid = int(ids[k + 1]) if 0 <= k < len(ids) - 1 else -1
    return (oid, int(ids[0])) if s else (int(ids[0]), oid)


def game_log_host(plies: Sequence[Mapping], *, num_envs: int, max_ply: int, capacity: int, start_state=None, pairs=None,
                  pair_stride: int = 0, envs_per_pair: int = 1, ids=None) -> HostGameLog:
    """Run a script of plies through ``HostGameLog`` from ``begin``.  A ply is a mapping with ``actions``, ``rewards``,
    ``terminated``, ``truncated``, ``pre_players`` and optionally ``reason``, ``n_legal``, ``live``, ``state`` (the env
    state rows after the step; default ``start_state``), ``ply_counter`` (default: the ply's index) and ``seat`` =
    ``(jobs, slots, envs_per_slot)``, applied before the ply as the arena seats at a sync point.  ``start_state``: the
    (E, >= 96) uint8 rows games start from (default: the standard start).  Per-env players (``ka_gamelog_step_env``):
    ``ids`` here, or ``ids`` in a ply from which on they hold (a new cohort), and ``side`` / ``opp`` in every ply, the
    players who play it."""
    E = int(num_envs)
    if start_state is None:
        start_state = np.tile(_standard_start_row(), (E, 1))
    log = HostGameLog(E, max_ply, capacity)
    log.begin(start_state)
    for t, ply in enumerate(plies):
        if ply.get("seat") is not None:
            log.seat(*ply["seat"])
        if ply.get("ids") is not None:
            ids = ply["ids"]
        per_env = {} if ids is None else dict(side=ply["side"], opp=ply["opp"], ids=ids)
        log.step(ply.get("state", start_state), ply["actions"], ply["rewards"], ply["terminated"], ply["truncated"],
                 ply["pre_players"], ply.get("reason", np.zeros(E, np.uint8)), nlegal=ply.get("n_legal"),
                 live=ply.get("live"), pairs=pairs, pair_stride=pair_stride, envs_per_pair=envs_per_pair,
                 ply_counter=ply.get("ply_counter", t), **per_env)
    return log


# ---------------------------------------------------------------------------------------------- device
class GameLog:
    """The device-resident log of one ``VecEnv`` (see the module docstring).  ``capacity`` finished games fit between two
    ``drain()`` calls; a game beyond that is dropped whole and counted in ``dropped``.

    ``begin()`` follows ``env.reset()``; ``step(...)`` (or ``step_env(...)``, per-env players) follows ``env.step(...)``
    and precedes the owner's bookkeeping launch; ``live(...)`` reads the games in progress at a sync point;
    ``seat(jobs, n)`` follows ``ka_arena_assign`` (the arena's slots are ``envs_per_slot`` envs each); ``drain()`` runs at
    a sync point, outside any captured graph."""

    def __init__(self, env, *, capacity: int, device=None, envs_per_slot: Optional[int] = None) -> None:
        if capacity < 1:
            raise ValueError(f"capacity must be positive, got {capacity}")
        self.env, self.capacity = env, int(capacity)
        self.device = torch.device(device) if device is not None else env.device
        if self.device != env.device:
            raise ValueError(f"the log lives with its env on {env.device}, got {self.device}")
        E, P = int(env._n), int(env._max_ply)
        top = _lib.query("ka_gamelog_words", 6, 0)
        if not 1 <= E <= top:
            raise ValueError(f"a game log covers 1..{top} envs, the env has {E}")
        if not 1 <= P <= 65535:
            raise ValueError(f"a game log needs an env with max_ply in [1, 65535], got {P}")
        words = _lib.query("ka_gamelog_words", 0, P)
        if (words, _lib.query("ka_gamelog_words", 1, 0), _lib.query("ka_gamelog_words", 2, 0),
                _lib.query("ka_gamelog_words", 4, 0), _lib.query("ka_gamelog_words", 5, 0)) != \
                (record_words(P), CURSOR_WORDS, META_WORDS, HEAD_WORDS, START_WORDS):
            raise _lib.KeiseiHipError("libkeisei_amd.so and keisei_amd.training.game_log disagree on the game log layout: "
                                      "rebuild the library")
        if self.capacity * words >= 1 << 31:
            raise ValueError(f"capacity {capacity} x {words} words does not fit the log's 32-bit indices")
        self.num_envs, self.max_ply, self.row_stride = E, P, 2 * ((P + 1) // 2)
        if envs_per_slot is not None and (envs_per_slot < 1 or E % envs_per_slot):
            raise ValueError(f"envs_per_slot ({envs_per_slot}) must divide the env's {E} envs")
        self.envs_per_slot = envs_per_slot
        self._state_bytes = int(env._state.shape[1])
        dev = self.device
        with torch.cuda.device(dev):
            z = lambda *s, dtype=torch.int32: torch.zeros(*s, dtype=dtype, device=dev)  # noqa: E731
            self._rows = z(E, self.row_stride, dtype=torch.int16)        # a uint16 payload
            self._meta, self._starts = z(E, META_WORDS), z(E, START_WORDS)
            self._records = z(self.capacity, words)
            self._cursor = z(CURSOR_WORDS)
        self._records_host = torch.zeros(self.capacity, words, dtype=torch.int32).pin_memory()
        self._cursor_host = torch.zeros(CURSOR_WORDS, dtype=torch.int32).pin_memory()
        self.dropped = 0
        self.plies_logged = 0

    @property
    def nbytes(self) -> int:
        return sum(t.numel() * t.element_size() for t in (self._rows, self._meta, self._starts, self._records, self._cursor))

    def begin(self) -> None:
        """Every env's game starts now, from what its state row holds; the cursor and the counters are cleared."""
        with torch.cuda.device(self.device):
            self._cursor.zero_()
            _lib.call("ka_gamelog_begin", self.env._state, self._state_bytes, self.num_envs, self._meta, self._starts,
                      _lib.stream_ptr(self.device))
        self.dropped = self.plies_logged = 0

    def step(self, actions, rewards, terminated, truncated, pre_player, reason, *, nlegal=None, live=None, pairs=None,
             pair_stride: int = 0, envs_per_pair: int = 1, ply_counter=None) -> None:
        """One launch on the current stream.  Tensors or raw device pointers; see ``ka_gamelog_step`` in the header."""
        _lib.call("ka_gamelog_step", self.env._state, self._state_bytes, self.num_envs, self.max_ply, actions, rewards,
                  terminated, truncated, pre_player, reason, nlegal, live, pairs, int(pair_stride), int(envs_per_pair),
                  ply_counter, self._rows, self.row_stride, self._meta, self._starts, self._records, self.capacity,
                  self._cursor, _lib.stream_ptr(self.device))

    def step_env(self, actions, rewards, terminated, truncated, pre_player, reason, *, side, opp, ids, opponents: int,
                 nlegal=None, live=None, ply_counter=None) -> None:
        """One launch on the current stream with the players per env: ``side`` (E u8, the learner's colour), ``opp`` (E
        int32, the opponent's index), ``ids`` (``opponents`` + 1 int32 on the device: the learner's id, then the
        opponents').  See ``ka_gamelog_step_env`` in the header."""
        _lib.call("ka_gamelog_step_env", self.env._state, self._state_bytes, self.num_envs, self.max_ply, actions, rewards,
                  terminated, truncated, pre_player, reason, nlegal, live, side, opp, ids, int(opponents), ply_counter,
                  self._rows, self.row_stride, self._meta, self._starts, self._records, self.capacity, self._cursor,
                  _lib.stream_ptr(self.device))

    def live(self, envs=None, *, pairs=None, pair_stride: int = 0, envs_per_pair: int = 1, side=None, opp=None, ids=None,
             opponents: Optional[int] = None, ply_counter=None) -> List[RecordedGame]:
        """Sync point: the games in progress of ``envs`` (default: every env, in env order) as ``RecordedGame`` with
        ``finished=False``, ``winner=-1`` and ``end_ply`` = the owner's ply counter now.  One launch (``ka_gamelog_peek``)
        and one copy of exactly the rows asked for; the log is not changed.  The players as ``step`` (``pairs``) or
        ``step_env`` (``side`` / ``opp`` / ``ids``) takes them, or neither."""
        if pairs is not None and side is not None:
            raise ValueError("the players come from pairs or from side / opp / ids, not both")
        if side is not None:
            if opp is None or ids is None:
                raise ValueError("per-env players need side, opp and ids together")
            opponents = int(ids.numel()) - 1 if opponents is None else int(opponents)
        with torch.cuda.device(self.device):
            lst, n = None, self.num_envs
            if envs is not None:
                host = np.asarray(envs, dtype=np.int64).reshape(-1)
                if host.size and (host.min() < 0 or host.max() >= self.num_envs):
                    raise ValueError(f"envs must lie in [0, {self.num_envs}), got {host.tolist()}")
                lst, n = torch.from_numpy(host.astype(np.int32)).to(self.device), int(host.size)
            if n == 0:
                return []
            words = record_words(self.max_ply)
            out = torch.empty(n, words, dtype=torch.int32, device=self.device)
            _lib.call("ka_gamelog_peek", lst, n, self.num_envs, self.max_ply, pairs, int(pair_stride), int(envs_per_pair),
                      side, opp, ids, int(opponents or 0), ply_counter, self._rows, self.row_stride, self._meta, self._starts,
                      out, _lib.stream_ptr(self.device))
            return games_from_records(out.cpu().numpy())

    def seat(self, jobs, n: int) -> None:
        """Behind ``ka_arena_assign`` with the same ``n`` jobs (a log built with ``envs_per_slot``): the games in progress
        in those slots are carried."""
        if self.envs_per_slot is None:
            raise ValueError("seat() needs a GameLog built with envs_per_slot")
        _lib.call("ka_gamelog_seat", jobs, int(n), self.num_envs // self.envs_per_slot, self.envs_per_slot, self._meta,
                  _lib.stream_ptr(self.device))

    def drain(self) -> List[RecordedGame]:
        """Sync point: one read of the cursor, one copy of exactly the committed records, the cursor zeroed."""
        with torch.cuda.device(self.device):
            self._cursor_host.copy_(self._cursor)
            n, lost, plies, _ = (int(v) for v in self._cursor_host)
            self.dropped += lost
            self.plies_logged += plies
            games: List[RecordedGame] = []
            if n:
                self._records_host[:n].copy_(self._records[:n])
                games = games_from_records(self._records_host[:n].numpy())
            if n or lost or plies:
                self._cursor.zero_()
        return games
