"""SL data preparation: game records -> real position shards, replayed on the device (keisei/sl/prepare.py, with the four
steps its placeholder leaves out, :151-161: replay the moves, observe every position, encode the played move with the
spatial action mapper, take the material balance for the score head).

    python -m keisei_amd.sl.prepare --sources games/ --output shards/ [--min-ply 40] [--min-rating R] [--shard-size N]

File handling is the reference's: the same file discovery, stale shards and metadata removed first, one bad record does
not lose the file, ``shard_meta.json`` written atomically, shard k holds positions [k * S, (k + 1) * S) so the cap can
fall inside a game.  What differs is where a position comes from:

  host    ``usi_to_action``: USI text -> spatial action index, no board needed (the mover is the ply parity).  A batch of
          games becomes one int32 action stream plus per-game offset / length / outcome / first shard row (``ReplayBatch``).
  device  game g of a batch sits in env g of a ``VecEnv``; all envs step in lockstep from ``reset()``.  One ply is
          ``ka_sl_replay_plan`` -> ``ka_shogi_env_step`` -> ``ka_sl_replay_record`` (csrc/sl_prepare.hip): the record kernel
          writes the finished 16 220-byte record -- observation before the move, policy index, W/D/L for the mover, material
          after the move / 76 -- straight into the shard buffer.  No host read until the batch is through; then one read of
          the state and one copy of the buffer.

A game is cut, keeping the positions before the cut, at a move that has no spatial encoding or is not legal, where the
rules end it before the record does, and at ``max_moves``.  Only games from the standard start position are replayed.

``prepare_sl_dataset`` is the same preparation without the disk (not in the reference): the same games, batches, cuts and
counters, but the kept records of every batch are packed from the replay's device buffer straight onto a
``keisei_amd.sl.device_dataset.DeviceSLDataset``; no shard file, no pinned copy, no ``shard_meta.json``.

``_replay_host`` is the same bookkeeping in numpy over any VecEnv-shaped object (the CPU oracle in the tests): the
yardstick the kernels are held to.
"""
from __future__ import annotations

import argparse
import json
import logging
import re
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, Iterator, List, Optional, Sequence, Tuple

import numpy as np
import torch

from keisei_amd import _lib
from keisei_amd.shogi_gym import ACTION_SPACE, MASK_WORDS, SpatialActionMapper
from keisei_amd.sl.dataset import OBS_SIZE, RECORD_SIZE, SCORE_NORMALIZATION, _RECORD
from keisei_amd.sl.parsers import (CSAParser, GameFilter, GameOutcome, GameParser, GameRecord, SFENParser,
                                   is_standard_start)

logger = logging.getLogger(__name__)

__all__ = ["prepare_sl_data", "prepare_sl_dataset", "dataset_from_recorded_games", "opening_positions", "usi_to_action", "ReplayBatch", "main"]

# why a game's record was not used to its end
REASON_NONE, REASON_ILLEGAL, REASON_RULES, REASON_LONG, REASON_NO_ENCODING = 0, 1, 2, 3, 4
_OUTCOME = {GameOutcome.WIN_BLACK: 0, GameOutcome.WIN_WHITE: 1, GameOutcome.DRAW: 2}
_SENTINEL = 0xA5
# header words of the device state (csrc/sl_prepare.hip)
_PLIES, _WRITTEN, _FILLER, _ILLEGAL, _RULES, _STALL, _REFUSAL = 0, 1, 2, 3, 4, 5, 6

_BOARD_MOVE = re.compile(r"^([1-9])([a-i])([1-9])([a-i])(\+?)$")
_DROP_MOVE = re.compile(r"^([PLNSGBR])\*([1-9])([a-i])$")
_HAND = "PLNSGBR"
_MAPPER = SpatialActionMapper()


# ---------------------------------------------------------------------------------------------- USI -> action stream
def _square(file_ch: str, rank_ch: str) -> int:
    """Row-major square of VecEnv.get_sfen: rank 'a' is row 0, file 9 is column 0."""
    return (ord(rank_ch) - ord("a")) * 9 + (9 - int(file_ch))


def usi_to_action(move_usi: str, is_white: bool) -> int:
    """The spatial action index of a USI move (``7g7f``, ``2b3c+``, ``P*5e``) for the side that plays it.  Raises
    ``ValueError`` for malformed text and for a move the 139 spatial planes cannot hold."""
    m = _DROP_MOVE.match(move_usi)
    if m:
        return _MAPPER.encode_drop_move(_square(m.group(2), m.group(3)), _HAND.index(m.group(1)), is_white)
    m = _BOARD_MOVE.match(move_usi)
    if not m:
        raise ValueError(f"not a USI move: {move_usi!r}")
    frm, to, promote = _square(m.group(1), m.group(2)), _square(m.group(3), m.group(4)), bool(m.group(5))
    idx = _MAPPER.encode_board_move(frm, to, promote, is_white)
    back = _MAPPER.decode(idx, is_white)                        # (a knight's jump backwards would alias a forward one)
    if (back["from_sq"], back["to_sq"], back["promote"]) != (frm, to, promote):
        raise ValueError(f"move {move_usi!r} has no spatial encoding")
    return idx


def _encode_game(record: GameRecord, max_moves: int) -> Tuple[np.ndarray, int]:
    """The record's moves as action indices, cut where a move cannot be encoded or at ``max_moves``; the host's reason."""
    out, reason = [], REASON_NONE
    for i, move in enumerate(record.moves):
        if i >= max_moves:
            reason = REASON_LONG
            break
        try:
            out.append(usi_to_action(move.move_usi, bool(i & 1)))
        except ValueError:
            reason = REASON_NO_ENCODING
            break
    return np.asarray(out, dtype=np.int32), reason


@dataclass
class ReplayBatch:
    """A batch of games for one lockstep replay.  Env e plays the game in slot e; slots are sorted by length (longest
    first), ``row_of`` is the prefix sum of the lengths in RECORD order, so the shard buffer is in the reference's loop
    order whatever the slot order.  ``order[e]`` is the record-order index of slot e's game, -1 for padding."""
    actions: np.ndarray          # int32 [max(total, 1)]
    offset: np.ndarray           # int32 [E]
    length: np.ndarray           # int32 [E]
    outcome: np.ndarray          # int32 [E]: 0 black wins, 1 white wins, 2 draw
    row_of: np.ndarray           # int32 [E]
    order: np.ndarray            # int32 [E]
    rows: int

    @property
    def num_envs(self) -> int:
        return int(self.length.shape[0])

    @classmethod
    def build(cls, games: Sequence[tuple]) -> "ReplayBatch":
        """``games``: (action indices, outcome 0 / 1 / 2, ...) per game, in record order."""
        games = [(g[0], g[1]) for g in games]
        lens = np.asarray([len(a) for a, _ in games], dtype=np.int64)
        start = np.concatenate(([0], np.cumsum(lens)))[:-1] if len(games) else np.zeros(0, np.int64)
        order = np.argsort(-lens, kind="stable")
        actions = np.concatenate([np.asarray(a, np.int32) for a, _ in games] + [np.zeros(0, np.int32)])
        if actions.size == 0:
            actions = np.zeros(1, np.int32)
        i32 = lambda x: np.ascontiguousarray(x, dtype=np.int32)  # noqa: E731
        return cls(actions=i32(actions), offset=i32(start[order]), length=i32(lens[order]),
                   outcome=i32(np.asarray([o for _, o in games], dtype=np.int64)[order]), row_of=i32(start[order]),
                   order=i32(order), rows=int(lens.sum()))

    def padded(self, num_envs: int) -> "ReplayBatch":
        """The batch over ``num_envs`` envs: the extra envs hold empty records and play fillers only."""
        pad = num_envs - self.num_envs
        if pad < 0:
            raise ValueError(f"a batch of {self.num_envs} games does not fit {num_envs} envs")
        if pad == 0:
            return self
        z = np.zeros(pad, np.int32)
        cat = lambda x, fill=z: np.concatenate([x, fill])  # noqa: E731
        return ReplayBatch(self.actions, cat(self.offset), cat(self.length), cat(self.outcome, z + 2), cat(self.row_of),
                           cat(self.order, z - 1), self.rows)


def _batches(games, batch_envs: int, max_batch_positions: int) -> Iterator[List]:
    """Consecutive games, at most ``batch_envs`` of them and ``max_batch_positions`` rows per batch."""
    cur, rows = [], 0
    for g in games:
        n = len(g[0])
        if cur and (len(cur) == batch_envs or rows + n > max_batch_positions):
            yield cur
            cur, rows = [], 0
        cur.append(g)
        rows += n
    if cur:
        yield cur


# ---------------------------------------------------------------------------------------------- host restatement
def _value_of(outcome: int, mover: int) -> int:
    """W / D / L = 0 / 1 / 2 for the side that moves (prepare.py:141-149)."""
    return 1 if outcome == 2 else (0 if outcome == mover else 2)


def _env_reset(env):
    r = env.reset()
    if isinstance(r, tuple):                                    # OracleVecEnv
        return r[0], np.asarray(r[1], dtype=bool)
    return np.asarray(r.observations), np.asarray(r.legal_masks, dtype=bool)


def _env_step(env, actions: np.ndarray) -> dict:
    r = env.step(actions)
    if isinstance(r, dict):                                     # OracleVecEnv
        return r
    return dict(observations=np.asarray(r.observations), legal_masks=np.asarray(r.legal_masks, dtype=bool),
                terminated=np.asarray(r.terminated), truncated=np.asarray(r.truncated),
                current_players=np.asarray(r.current_players), material_balance=np.asarray(r.step_metadata.material_balance))


def _replay_host(batch: ReplayBatch, env, rows: Optional[int] = None):
    """``ka_sl_replay_plan`` / ``ka_sl_replay_record`` in numpy over ``env`` (``reset()`` / ``step(actions)`` of a numpy
    ``VecEnv`` or of the CPU oracle; as many envs as the batch has slots, ``max_ply`` as the device env's).
    Returns ``(buffer, valid_len, reason, header)``: the shard buffer as ``rows`` structured records whose unwritten rows
    are 0xA5 bytes, the per-slot cut and its reason, the header counters of the device state."""
    E = batch.num_envs
    rows = batch.rows if rows is None else rows
    raw = np.full((rows, RECORD_SIZE), _SENTINEL, dtype=np.uint8)
    buf = raw.reshape(-1).view(_RECORD)
    valid_len, reason = batch.length.copy(), np.zeros(E, np.int32)
    hdr = np.zeros(8, np.int64)
    obs, mask = _env_reset(env)
    players = np.zeros(E, np.uint8)                             # black moves first
    for i in range(int(batch.length.max()) if E else 0):
        hdr[_RULES] += int(((reason == REASON_RULES) & (valid_len == i)).sum())
        live = i < valid_len
        mv = np.where(live, batch.actions[np.minimum(batch.offset.astype(np.int64) + i, batch.actions.size - 1)], -1)
        legal = live & (mv >= 0) & (mv < ACTION_SPACE)
        legal[legal] = mask[np.nonzero(legal)[0], mv[legal]]
        cut = live & ~legal
        valid_len[cut], reason[cut] = i, REASON_ILLEGAL
        hdr[_ILLEGAL] += int(cut.sum())
        if not mask.any(axis=1).all():
            hdr[_STALL] += int((~mask.any(axis=1)).sum())
        act = np.where(legal, mv, mask.argmax(axis=1)).astype(np.int64)     # the filler: the lowest legal action
        hdr[_PLIES] += 1
        hdr[_WRITTEN] += int(legal.sum())
        hdr[_FILLER] += int(E - legal.sum())
        r = _env_step(env, act)
        material = np.asarray(r["material_balance"]).astype(np.float32) / np.float32(SCORE_NORMALIZATION)
        for e in np.nonzero(legal)[0]:
            row = int(batch.row_of[e]) + i
            if not 0 <= row < rows:
                continue
            rec = buf[row:row + 1]
            rec["obs"] = obs[e].reshape(1, OBS_SIZE)            # the position the move was played IN
            rec["policy"], rec["value"] = int(act[e]), _value_of(int(batch.outcome[e]), int(players[e]) & 1)
            rec["score"] = material[e]
        done = np.asarray(r["terminated"], dtype=bool) | np.asarray(r["truncated"], dtype=bool)
        ended = legal & done & (i + 1 < valid_len)              # the env has restarted the game: the record goes no further
        valid_len[ended], reason[ended] = i + 1, REASON_RULES
        obs, mask, players = r["observations"], np.asarray(r["legal_masks"], dtype=bool), np.asarray(r["current_players"])
    return buf, valid_len, reason, hdr


def _kept_rows(batch: ReplayBatch, valid_len: np.ndarray) -> np.ndarray:
    """Which rows of the batch's buffer hold a record: the first valid_len rows of every game."""
    keep = np.zeros(batch.rows, dtype=bool)
    for e in range(batch.num_envs):
        keep[int(batch.row_of[e]):int(batch.row_of[e]) + int(valid_len[e])] = True
    return keep


# ---------------------------------------------------------------------------------------------- device replay
class _DeviceReplay:
    """The env, the state and the shard buffer of the device replay (see the module docstring)."""

    def __init__(self, batch_envs: int, max_moves: int, device=None) -> None:
        from keisei_amd.shogi_gym import VecEnv                 # raises KeiseiHipError without the library or a GPU

        if _lib.available():
            top = _lib.query("ka_sl_replay_state_words", 2)
            if not 1 <= batch_envs <= top:
                raise ValueError(f"batch_envs must lie in [1, {top}], got {batch_envs}")
        if not 1 <= max_moves <= 65535:
            raise ValueError(f"max_moves must lie in [1, 65535] (the env's ply counter), got {max_moves}")
        self.num_envs, self.max_ply = int(batch_envs), int(max_moves)
        self.env = VecEnv(self.num_envs, self.max_ply, "katago", "spatial", device=device, output="torch", check_actions=False)
        self.device = self.env.device
        if _lib.query("ka_sl_replay_state_words", 3) != RECORD_SIZE or _lib.query("ka_sl_replay_state_words", 1) != 3:
            raise _lib.KeiseiHipError("libkeisei_amd.so and keisei_amd.sl.prepare disagree on the shard record or the replay "
                                      "state layout: rebuild the library")
        self._hdr = _lib.query("ka_sl_replay_state_words", 0)
        E, dev = self.num_envs, self.device
        with torch.cuda.device(dev):
            self._state = torch.zeros(self._hdr + 3 * E, dtype=torch.int32, device=dev)
            self._state_host = torch.zeros(self._hdr + 3 * E, dtype=torch.int32).pin_memory()
            self._games = torch.zeros(4, E, dtype=torch.int32, device=dev)
            self._act = torch.zeros(E, dtype=torch.int64, device=dev)
            self._write = torch.zeros(E, dtype=torch.int32, device=dev)
        self._shard: Optional[torch.Tensor] = None
        self._shard_host: Optional[torch.Tensor] = None

    def _buffers(self, nbytes: int) -> None:
        if self._shard is None or self._shard.numel() < nbytes:
            self._shard = self._shard_host = None
            with torch.cuda.device(self.device):
                self._shard = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._shard_host = torch.empty(nbytes, dtype=torch.uint8).pin_memory()

    def replay(self, batch: ReplayBatch, out: Optional[torch.Tensor] = None):
        """Replay one batch.  ``out``: a contiguous uint8 device tensor of ``batch.rows * 16220`` bytes to write into
        (tests); by default the replay's own buffer, copied to pinned host memory.
        Returns ``(buffer, valid_len, reason, header)`` like ``_replay_host``; ``buffer`` is None when ``out`` is given."""
        E = self.num_envs
        batch = batch.padded(E)
        rows, plies = batch.rows, int(batch.length.max())
        if (batch.length < 0).any() or (batch.offset < 0).any() or (batch.row_of < 0).any() or \
                int((batch.offset.astype(np.int64) + batch.length).max()) > batch.actions.size or \
                int((batch.row_of.astype(np.int64) + batch.length).max()) > rows or plies > self.max_ply:
            raise ValueError("ReplayBatch: offsets, lengths or rows do not fit the action stream, the buffer or max_moves")
        if rows == 0:
            return np.zeros(0, _RECORD), batch.length.copy(), np.zeros(E, np.int32), np.zeros(self._hdr, np.int64)
        nbytes = rows * RECORD_SIZE
        if out is None:
            self._buffers(nbytes)
            shard = self._shard
        else:
            if out.dtype != torch.uint8 or out.numel() != nbytes or not out.is_contiguous() or out.device != self.device:
                raise ValueError(f"out must be a contiguous uint8 tensor of {nbytes} bytes on {self.device}")
            shard = out
        env, dev = self.env, self.device
        with torch.cuda.device(dev):
            st = _lib.stream_ptr(dev)
            actions = torch.from_numpy(batch.actions).to(dev)
            self._games.copy_(torch.from_numpy(np.stack([batch.offset, batch.length, batch.outcome, batch.row_of])))
            init = np.zeros(self._hdr + 3 * E, np.int32)
            init[self._hdr + E:self._hdr + 2 * E] = batch.length
            self._state.copy_(torch.from_numpy(init))
            offset, outcome, row_of = self._games[0], self._games[2], self._games[3]
            env.reset()
            for _ in range(plies):
                prev = env._cur
                _lib.call("ka_sl_replay_plan", self._state, E, actions, int(actions.numel()), offset,
                          env._bits[prev], MASK_WORDS, self._act, self._write, st)
                env.step(self._act)
                nxt = env._cur
                # queued before the next ply's step, which overwrites the [prev] buffers
                _lib.call("ka_sl_replay_record", self._state, E, outcome, row_of, env._obs[prev], OBS_SIZE,
                          env._players[prev], self._act, self._write, env._material[nxt], env._terminated[nxt],
                          env._truncated[nxt], env._err.data_ptr() + 8, shard, rows, st)
            self._state_host.copy_(self._state)                  # the one read of the state
            host = self._state_host.numpy()
            hdr = host[:self._hdr].astype(np.int64)
            if hdr[_REFUSAL] or hdr[_REFUSAL + 1] or hdr[_STALL]:
                env.raise_if_refused()
                raise _lib.KeiseiHipError(f"SL replay: {int(hdr[_STALL])} positions without a legal action")
            valid_len = host[self._hdr + E:self._hdr + 2 * E].copy()
            reason = host[self._hdr + 2 * E:].copy()
            buf = None
            if out is None:
                self._shard_host[:nbytes].copy_(shard[:nbytes])
                buf = self._shard_host[:nbytes].numpy().view(_RECORD)
        return buf, valid_len, reason, hdr


# ---------------------------------------------------------------------------------------------- files
def _parsers_by_extension() -> Dict[str, GameParser]:
    """``{".sfen": SFENParser(), ".csa": CSAParser()}``; two parsers may not claim one extension."""
    by_ext: Dict[str, GameParser] = {}
    for parser in (SFENParser(), CSAParser()):
        clash = by_ext.keys() & parser.supported_extensions()
        if clash:
            raise ValueError(f"extension {sorted(clash)[0]!r} has two parsers")
        by_ext.update(dict.fromkeys(sorted(parser.supported_extensions()), parser))
    return by_ext


def _records_of(parser: GameParser, game_file: Path) -> Iterator[Optional[GameRecord]]:
    """The file's records, one by one.  A record that fails to parse comes out as None and the iteration goes on with the
    next one (a generator that raised is finished, so that ends the file); a file that cannot be opened is one None."""
    done = object()

    def step(records):
        try:
            return next(records, done)
        except Exception:
            logger.exception("%s: a game record could not be parsed and is left out", game_file)
            return None

    try:
        records = iter(parser.parse(game_file))
    except Exception:
        logger.exception("%s could not be read and is left out", game_file)
        yield None
        return
    record = step(records)
    while record is not done:
        yield record
        record = step(records)


def _discover(game_sources: Sequence[str], parsers: Dict[str, GameParser]) -> List[Path]:
    """A source that is a file is taken as it is; of a directory, the files directly in it with a parser's extension in
    lower or upper case (``game.CSA``), per extension in name order.  Anything else is passed over."""
    found: List[Path] = []
    for source in map(Path, game_sources):
        if source.is_file():
            found.append(source)
        elif source.is_dir():
            for ext in parsers:
                for spelling in dict.fromkeys((ext, ext.upper())):
                    found += sorted(source.glob("*" + spelling))
    return found


class _ShardWriter:
    """Appends records and writes ``shard_<k>.bin`` whenever ``shard_size`` of them are waiting: shard k holds positions
    [k * S, (k + 1) * S) of the stream."""

    def __init__(self, output_path: Path, shard_size: int) -> None:
        if shard_size < 1:
            raise ValueError(f"shard_size must be positive, got {shard_size}")
        self.path, self.shard_size = output_path, int(shard_size)
        self.num_shards = self.num_positions = 0
        self._pending: List[np.ndarray] = []
        self._count = 0

    def append(self, records: np.ndarray) -> None:
        """``records``: structured rows of the shard layout; copied if they have to wait."""
        self.num_positions += len(records)
        while len(records):
            take = records[:self.shard_size - self._count]
            records = records[len(take):]
            self._count += len(take)
            if self._count == self.shard_size:
                self._flush(take)
            else:
                self._pending.append(take.copy())

    def _flush(self, last: Optional[np.ndarray] = None) -> None:
        parts = self._pending + ([last] if last is not None else [])
        if not sum(len(p) for p in parts):
            return
        name = self.path / f"shard_{self.num_shards:03d}.bin"
        with open(name, "wb") as f:
            for p in parts:
                np.ascontiguousarray(p).tofile(f)
        logger.info("Wrote shard %s with %d positions", name.name, self._count)
        self.num_shards += 1
        self._pending, self._count = [], 0

    def close(self) -> None:
        self._flush()


def prepare_sl_data(game_sources: List[str], output_dir: str, min_ply: int = 40, min_rating: Optional[int] = None,
                    shard_size: int = 100_000, *, device=None, batch_envs: int = 512, max_moves: int = 512,
                    max_batch_positions: int = 65536) -> dict:
    """Parse game records, replay them on the device and write position shards.  Returns what ``shard_meta.json`` holds."""
    if not 1 <= max_moves <= 65535:
        raise ValueError(f"max_moves must lie in [1, 65535] (the env's ply counter), got {max_moves}")
    if max_batch_positions < max_moves:
        raise ValueError(f"max_batch_positions ({max_batch_positions}) must hold one game of max_moves ({max_moves})")
    replay = _DeviceReplay(batch_envs, max_moves, device)       # raises KeiseiHipError without a GPU, before a file is touched
    return _prepare(game_sources, output_dir, GameFilter(min_ply=min_ply, min_rating=min_rating), shard_size, replay.replay,
                    batch_envs=batch_envs, max_moves=max_moves, max_batch_positions=max_batch_positions)


def _new_counters() -> dict:
    return dict(games=0, skipped=0, parse_errors=0, illegal=0, rules=0, long=0, nonstandard=0, filler=0, steps=0)


def _game_batches(game_sources: Sequence[str], game_filter: GameFilter, count: dict, *, batch_envs: int, max_moves: int,
                  max_batch_positions: int) -> Iterator[List[tuple]]:
    """The game iteration of ``prepare_sl_data`` and ``prepare_sl_dataset``: discover the files, parse and filter the
    records, encode the accepted games as ``(actions, outcome, host reason)`` and hand them out in replay batches.
    ``count`` is counted into while the batches are drawn."""
    parsers = _parsers_by_extension()
    game_files = _discover(game_sources, parsers)
    logger.info("%d game files in %d sources", len(game_files), len(game_sources))

    def accepted() -> Iterator[tuple]:
        for game_file in game_files:
            parser = parsers.get(game_file.suffix.lower())
            if parser is None:
                logger.warning("%s: no parser reads '%s' files, left out", game_file, game_file.suffix.lower())
                continue
            for record in _records_of(parser, game_file):
                if record is None:
                    count["parse_errors"] += 1
                elif not game_filter.accepts(record):
                    count["skipped"] += 1
                elif not is_standard_start(record.start):
                    count["nonstandard"] += 1
                else:
                    count["games"] += 1
                    actions, why = _encode_game(record, max_moves)
                    count["long"] += int(why == REASON_LONG)
                    yield actions, _OUTCOME[record.outcome], why

    return _batches(accepted(), batch_envs, max_batch_positions)


def _count_replay(count: dict, games: List[tuple], batch: ReplayBatch, reason: np.ndarray, hdr: np.ndarray) -> None:
    """What one replayed batch adds to the counters: the cuts (the device's reason, else the host's) and the fillers."""
    host_reason = np.asarray([g[2] for g in games], np.int32)[batch.order]
    final = np.where(reason[:len(games)] != REASON_NONE, reason[:len(games)], host_reason)
    count["illegal"] += int(((final == REASON_ILLEGAL) | (final == REASON_NO_ENCODING)).sum())
    count["rules"] += int((final == REASON_RULES).sum())
    count["filler"] += int(hdr[_FILLER])
    count["steps"] += int(hdr[_FILLER] + hdr[_WRITTEN])


def _meta_of(count: dict, num_positions: int, num_shards: Optional[int] = None) -> dict:
    meta = {"placeholder": False, "num_shards": num_shards, "num_games": count["games"],
            "num_positions": num_positions, "games_cut_illegal": count["illegal"],
            "games_cut_by_rules": count["rules"], "games_cut_long": count["long"],
            "games_nonstandard_start": count["nonstandard"]}
    if num_shards is None:
        del meta["num_shards"]
    return meta


def _log_summary(what: str, num_positions: int, count: dict) -> None:
    logger.info("Prepared %s (%d positions) from %d games: %d skipped by filter, %d parse errors, %d not from the "
                "standard start; cut: %d illegal, %d by the rules, %d long; %d of %d env steps were fillers",
                what, num_positions, count["games"], count["skipped"], count["parse_errors"],
                count["nonstandard"], count["illegal"], count["rules"], count["long"], count["filler"], count["steps"])


def _prepare(game_sources: Sequence[str], output_dir: str, game_filter: GameFilter, shard_size: int, replay, *,
             batch_envs: int, max_moves: int, max_batch_positions: int) -> dict:
    """Everything of ``prepare_sl_data`` around the replay; ``replay(batch)`` is ``_DeviceReplay.replay`` (or, in the CPU
    tests, ``_replay_host`` over the oracle)."""
    out = Path(output_dir)
    out.mkdir(parents=True, exist_ok=True)
    meta_path = out / "shard_meta.json"
    # what an earlier run left goes first: SLDataset reads every shard_*.bin it finds, and this run may write fewer
    for old in [*out.glob("shard_*.bin"), meta_path]:
        old.unlink(missing_ok=True)

    writer = _ShardWriter(out, shard_size)
    count = _new_counters()
    for games in _game_batches(game_sources, game_filter, count, batch_envs=batch_envs, max_moves=max_moves,
                               max_batch_positions=max_batch_positions):
        batch = ReplayBatch.build(games)
        buf, valid_len, reason, hdr = replay(batch)
        _count_replay(count, games, batch, reason, hdr)
        if batch.rows:
            writer.append(buf[_kept_rows(batch, valid_len)])
    writer.close()

    meta = _meta_of(count, writer.num_positions, writer.num_shards)
    # written beside the target and moved over it: a reader sees the old metadata, none, or all of the new
    partial = out / "shard_meta.json.tmp"
    partial.write_text(json.dumps(meta, indent=2) + "\n")
    partial.replace(meta_path)
    _log_summary(f"{writer.num_shards} shards", writer.num_positions, count)
    return meta


def _replay_onto(dataset, replay: _DeviceReplay, batch: ReplayBatch, raw: Optional[torch.Tensor]):
    """Replay one batch into the reused device buffer ``raw`` (grown when the batch needs more) and pack its kept records
    onto ``dataset``; the records never leave the device.  Returns ``(raw, reason, header)``."""
    if batch.rows == 0:
        return raw, np.zeros(batch.num_envs, np.int32), np.zeros(8, np.int64)
    nbytes = batch.rows * RECORD_SIZE
    if raw is None or raw.numel() < nbytes:
        raw = None
        with torch.cuda.device(replay.device):
            raw = torch.empty(nbytes, dtype=torch.uint8, device=replay.device)
    _, valid_len, reason, hdr = replay.replay(batch, out=raw[:nbytes])         # valid_len: the one read of the state
    dataset.append_raw(raw[:nbytes], np.nonzero(_kept_rows(batch, valid_len))[0])
    return raw, reason, hdr


def prepare_sl_dataset(game_sources: Sequence[str], min_ply: int = 40, min_rating: Optional[int] = None, *, device=None,
                       batch_envs: int = 512, max_moves: int = 512, max_batch_positions: int = 65536):
    """``prepare_sl_data`` without the disk: the same games, filters, batches, cuts and counters, but every replayed batch
    stays on the device and its kept records are packed straight onto a ``DeviceSLDataset``.  Returns ``(dataset, meta)``;
    ``meta`` holds the keys of ``shard_meta.json`` except ``num_shards``."""
    from keisei_amd.sl.device_dataset import DeviceSLDataset

    if not 1 <= max_moves <= 65535:
        raise ValueError(f"max_moves must lie in [1, 65535] (the env's ply counter), got {max_moves}")
    if max_batch_positions < max_moves:
        raise ValueError(f"max_batch_positions ({max_batch_positions}) must hold one game of max_moves ({max_moves})")
    replay = _DeviceReplay(batch_envs, max_moves, device)
    dataset = DeviceSLDataset(replay.device)
    raw: Optional[torch.Tensor] = None                          # the reused record buffer of a batch
    count = _new_counters()
    for games in _game_batches(game_sources, GameFilter(min_ply=min_ply, min_rating=min_rating), count,
                               batch_envs=batch_envs, max_moves=max_moves, max_batch_positions=max_batch_positions):
        batch = ReplayBatch.build(games)
        raw, reason, hdr = _replay_onto(dataset, replay, batch, raw)
        _count_replay(count, games, batch, reason, hdr)
    dataset.check()
    meta = _meta_of(count, len(dataset))
    _log_summary("a device dataset", len(dataset), count)
    return dataset, meta


def dataset_from_recorded_games(games, *, device=None, batch_envs: int = 512, max_moves: int = 512,
                                max_batch_positions: int = 65536):
    """A ``DeviceSLDataset`` straight from games a ``GameLog`` recorded (``keisei_amd.training.game_log.RecordedGame``:
    ``actions``, ``winner``, ``is_standard_start``): the replay of ``prepare_sl_dataset`` without the text -- no USI, no
    file, no new kernel.  The recorded action indices are the replay's action stream as they are.  Only games from the
    standard start are replayed; the others are counted in ``games_nonstandard_start``, a game without a move is passed
    over, a game still in progress (``live_games()``: no winner yet) raises ``ValueError``.  ``max_moves`` is the replay
    env's ``max_ply`` as in ``prepare_sl_dataset`` (a longer game is cut there and
    counted): the observation's ply plane is ply / max_ply, so pass the ``max_ply`` the games were played with to get the
    observations their players saw.  Positions are in the order of ``games``.  Returns ``(dataset, meta)`` with the keys
    of ``prepare_sl_dataset``."""
    from keisei_amd.sl.device_dataset import DeviceSLDataset

    if batch_envs < 1:
        raise ValueError(f"batch_envs must be positive, got {batch_envs}")
    if not 1 <= max_moves <= 65535:
        raise ValueError(f"max_moves must lie in [1, 65535] (the env's ply counter), got {max_moves}")
    if max_batch_positions < max_moves:
        raise ValueError(f"max_batch_positions ({max_batch_positions}) must hold one game of max_moves ({max_moves})")
    count = _new_counters()
    kept: List[tuple] = []
    games = list(games)
    for g in games:
        if not getattr(g, "finished", True):
            raise ValueError(f"the game in progress in env {g.env} (game {g.game_number}) has no winner yet: a dataset's value "
                             "targets need one; pass finished games (drained ones, not live_games())")
    for g in games:
        if not g.is_standard_start:
            count["nonstandard"] += 1
        elif len(g.actions):
            count["games"] += 1
            actions = np.asarray(g.actions).astype(np.int32)
            count["long"] += int(len(actions) > max_moves)
            kept.append((actions[:max_moves], int(g.winner), REASON_LONG if len(actions) > max_moves else REASON_NONE))
    replay = _DeviceReplay(min(int(batch_envs), max(len(kept), 1)), max_moves, device)
    dataset = DeviceSLDataset(replay.device)
    raw: Optional[torch.Tensor] = None
    for batch_games in _batches(iter(kept), replay.num_envs, max_batch_positions):
        batch = ReplayBatch.build(batch_games)
        raw, reason, hdr = _replay_onto(dataset, replay, batch, raw)
        _count_replay(count, batch_games, batch, reason, hdr)
    dataset.check()
    meta = _meta_of(count, len(dataset))
    _log_summary("a device dataset from recorded games", len(dataset), count)
    return dataset, meta


def opening_positions(game_sources: Sequence[str], ply: int, min_ply: int = 40, min_rating: Optional[int] = None, *,
                      max_positions: Optional[int] = None, device=None, batch_envs: int = 512):
    """Start positions for ``VecEnv.set_start_positions`` from game records (not in the reference): the position after
    ``ply`` moves of every game that ``prepare_sl_data`` would replay (same discovery, parsing and filter; standard start
    only), as ``(boards (K, 81), hands (K, 2, 7), sides (K,))`` uint8 arrays.  The games are replayed in lockstep on the
    device env; a game counts when its record has at least ``ply`` moves, all of them encodable and legal, and the rules
    have not ended it by then.  Duplicates are dropped by exact bytes, the first seen is kept, in record order;
    ``max_positions`` stops the replay once that many are found."""
    from keisei_amd.shogi_gym import POOL_ROW_BYTES, VecEnv

    if not 0 <= ply < 65535:
        raise ValueError(f"ply must lie in [0, 65535), got {ply}")
    if batch_envs < 1:
        raise ValueError(f"batch_envs must be positive, got {batch_envs}")
    if max_positions is not None and max_positions < 1:
        raise ValueError(f"max_positions must be positive, got {max_positions}")
    env = VecEnv(batch_envs, ply + 1, "katago", "spatial", device=device, output="torch", check_actions=False)
    dev, E = env.device, int(batch_envs)
    count = _new_counters()
    seen, rows = set(), []
    full = lambda: max_positions is not None and len(rows) >= max_positions  # noqa: E731
    for games in _game_batches(game_sources, GameFilter(min_ply=min_ply, min_rating=min_rating), count, batch_envs=E,
                               max_moves=max(ply, 1), max_batch_positions=E * max(ply, 1)):
        acts = np.zeros((E, max(ply, 1)), np.int64)
        alive = np.zeros(E, bool)
        for e, (a, _, _) in enumerate(games):
            if len(a) >= ply:
                acts[e, :ply], alive[e] = a[:ply], True
        with torch.cuda.device(dev):
            acts_d, alive_d = torch.from_numpy(acts).to(dev), torch.from_numpy(alive).to(dev)
            env.reset()
            ar = torch.arange(E, device=dev)
            for i in range(ply):
                cur = env.current()
                a = acts_d[:, i]
                legal = ((cur.legal_mask_bits[ar, a >> 5] >> (a & 31)) & 1).bool()
                alive_d &= legal
                filler = cur.legal_masks.to(torch.uint8).argmax(dim=1)       # a dead env plays on: the lowest legal action
                r = env.step(torch.where(alive_d, a, filler))
                alive_d &= ~(r.terminated | r.truncated)
            state = env._state[:, :POOL_ROW_BYTES].cpu().numpy()
            keep = alive_d.cpu().numpy()
            env.raise_if_refused()
        for e in np.nonzero(keep)[0]:
            key = state[e].tobytes()
            if key not in seen and not full():
                seen.add(key)
                rows.append(state[e].copy())
        if full():
            break
    out = np.stack(rows) if rows else np.zeros((0, POOL_ROW_BYTES), np.uint8)
    logger.info("%d opening positions at ply %d from %d games", len(rows), ply, count["games"])
    return out[:, :81].copy(), out[:, 81:95].reshape(-1, 2, 7).copy(), out[:, 95].copy()


def main(argv: Optional[Sequence[str]] = None) -> None:
    """``python -m keisei_amd.sl.prepare``: the reference's command line (same options and defaults)."""
    cli = argparse.ArgumentParser(prog="python -m keisei_amd.sl.prepare",
                                  description="Replay .sfen / .csa game records on the GPU and write SL position shards")
    cli.add_argument("--sources", nargs="+", required=True, metavar="PATH", help="game record files, or directories of them")
    cli.add_argument("--output", required=True, metavar="DIR", help="where shard_*.bin and shard_meta.json go")
    cli.add_argument("--min-ply", type=int, default=40, help="leave out games with fewer moves")
    cli.add_argument("--min-rating", type=int, default=None, help="leave out games that state a lower rating")
    cli.add_argument("--shard-size", type=int, default=100_000, help="positions per shard file")
    opt = cli.parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(name)s %(message)s")
    prepare_sl_data(opt.sources, opt.output, min_ply=opt.min_ply, min_rating=opt.min_rating, shard_size=opt.shard_size)


if __name__ == "__main__":
    main()
