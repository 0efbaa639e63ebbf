"""The SL position dataset held packed in device memory (csrc/sl_data.hip; an addition the reference does not have).

Every channel of a shard record's observation is a 0/1 piece plane or a spatially constant plane, so three mask words and
one value word per channel reproduce its 4050 floats bit for bit: a packed record is 204 dwords (816 bytes, the layout is
in include/keisei_amd.h) instead of 16 220 bytes.  ``DeviceSLDataset`` keeps the whole dataset that way in ONE device
allocation; a minibatch is one ``ka_sl_gather`` launch that decodes the rows of an index tensor into the fp32 NCHW
observations and the targets ``SLDataset.read_batch`` would give -- no memory map, no pinned copy, no upload per batch.

It is filled from a shard directory (``from_shards``: the files stream through two pinned staging buffers and are packed
on arrival) or from records that are already on the device (``append_raw``: the growth path of
``keisei_amd.sl.prepare.prepare_sl_dataset``, which never touches the disk).  A record that cannot be held packed, or whose
targets ``SLDataset`` would refuse, is never stored in altered form: the load raises.

``pack_records`` / ``unpack_records`` are the two kernels in numpy: the yardstick the GPU tests hold them to, byte for byte.

Shogi's rules are symmetric under the left-right reflection of the board (files reversed, ranks kept), so a reflected
position with the reflected move is as valid a sample as the original.  ``gather(..., mirror=)`` decodes rows reflected
(``ka_sl_gather_aug``: another mask bit per square and a closed form on the policy target; no second copy of the corpus);
``mirror_action`` / ``mirror_records`` / ``sl_mirror_draw`` restate it in numpy.  ``view(start, stop)`` is a read-only
dataset over a range of the same memory: shards keep game order, so a tail range is a held-out set of whole games.

A dataset may hold, beside every position, a *visit row* -- eight words ``action | visits << 16``, the visit counts a
visit-count search left over the position's root candidates -- and an *info row* (who played the move, in which game): the
samples ``keisei_amd.training.search_samples.SearchSamples.drain()`` appends through ``append_packed``.  It has them for every
position or for none.  ``gather(..., visit_targets=True)`` hands the visit distribution out as ``visit_actions`` /
``visit_weights`` (``ka_sl_gather_visits``, reflected with the position); ``visit_weights`` / ``mirror_visit_words`` restate it.
"""
from __future__ import annotations

from pathlib import Path
from typing import Callable, List, Optional, Tuple

import numpy as np
import torch

from keisei_amd import _lib
from keisei_amd.sl.dataset import NUM_ACTIONS, OBS_SIZE, RECORD_SIZE, SLDataset, _RECORD

__all__ = ["DeviceSLDataset", "pack_records", "unpack_records", "mirror_action", "mirror_records", "sl_mirror_draw",
           "visit_weights", "mirror_visit_words", "PACKED_WORDS", "PACKED_BYTES", "VISIT_SLOTS", "INFO_WORDS"]

PACKED_WORDS = 204                       # KA_SL_PACKED_WORDS
PACKED_BYTES = 4 * PACKED_WORDS
VISIT_SLOTS, INFO_WORDS = 8, 4           # a position's visit row (action | visits << 16 per slot) and its info row
_CHANNELS, _SQUARES = 50, 81
_VALUE_AT, _POLICY_AT = 3 * _CHANNELS, 4 * _CHANNELS
_INT_MAX = 2 ** 31 - 1
_M64 = 2 ** 64 - 1
_MIRROR_SALT = 0x6D6972726F72            # "mirror": the salt of ka_sl_gather_aug's draw
MIRROR_NONE, MIRROR_ALL, MIRROR_DRAWN = 0, 1, 2      # the modes of ka_sl_gather_aug
_UNPACKABLE = "channel values are not one-valued planes; this dataset cannot be held packed"


# ---------------------------------------------------------------------------------------------- host restatement
def _as_records(records) -> np.ndarray:
    rec = np.asarray(records)
    if rec.dtype != _RECORD:
        raise TypeError(f"records must have the shard record dtype, got {rec.dtype}")
    return rec.reshape(-1)


def _obs_bits(rec: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(rec["obs"]).view(np.uint32).reshape(len(rec), _CHANNELS, _SQUARES)


def record_faults(records) -> Tuple[np.ndarray, np.ndarray]:
    """``(unpackable, bad_target)``, one bool per record: some channel holds two different non-zero patterns; the policy
    lies outside [0, 11259) or the value outside {0, 1, 2} (the rule of ``SLDataset._check_targets``)."""
    rec = _as_records(records)
    bits = _obs_bits(rec)
    nonzero = bits != 0
    value = np.take_along_axis(bits, nonzero.argmax(axis=2)[..., None], axis=2)      # the lowest non-zero square's pattern
    unpackable = (nonzero & (bits != value)).any(axis=(1, 2))
    policy, val = rec["policy"], rec["value"]
    bad_target = (policy < 0) | (policy >= NUM_ACTIONS) | (val < 0) | (val > 2)
    return unpackable, bad_target


def pack_records(records) -> Tuple[np.ndarray, Optional[int]]:
    """``ka_sl_pack`` in numpy: ``(uint32[n, 204], first_bad)``.  ``first_bad`` is the lowest index of a record that is not
    packable or has an invalid target (``record_faults`` says which), None when there is none; such a record's packed row
    is what the kernel writes for it, not a faithful copy."""
    rec = _as_records(records)
    n = len(rec)
    bits = _obs_bits(rec)
    nonzero = bits != 0
    out = np.zeros((n, PACKED_WORDS), dtype=np.uint32)
    field = np.zeros((n, _CHANNELS, 96), dtype=np.uint32)
    field[:, :, :_SQUARES] = nonzero
    weights = np.uint32(1) << np.arange(32, dtype=np.uint32)
    out[:, :_VALUE_AT] = (field.reshape(n, _CHANNELS, 3, 32) * weights).sum(axis=3, dtype=np.uint32).reshape(n, _VALUE_AT)
    value = np.take_along_axis(bits, nonzero.argmax(axis=2)[..., None], axis=2)[..., 0]
    out[:, _VALUE_AT:_POLICY_AT] = np.where(nonzero.any(axis=2), value, 0)
    out[:, _POLICY_AT + 0] = rec["policy"].astype(np.int64).view(np.uint64).astype(np.uint32)      # the low dword
    out[:, _POLICY_AT + 1] = rec["value"].astype(np.int64).view(np.uint64).astype(np.uint32)
    out[:, _POLICY_AT + 2] = np.ascontiguousarray(rec["score"]).view(np.uint32)
    unpackable, bad_target = record_faults(rec)
    bad = np.nonzero(unpackable | bad_target)[0]
    return out, (int(bad[0]) if bad.size else None)


def unpack_records(packed) -> np.ndarray:
    """``ka_sl_gather`` in numpy: the shard records of packed rows ``uint32[n, 204]``."""
    pk = np.ascontiguousarray(packed, dtype=np.uint32).reshape(-1, PACKED_WORDS)
    n = len(pk)
    squares = np.arange(_SQUARES)
    words = pk[:, :_VALUE_AT].reshape(n, _CHANNELS, 3)[:, :, squares >> 5]            # (n, 50, 81): the word of square p
    mask = ((words >> (squares & 31).astype(np.uint32)) & np.uint32(1)).astype(bool)
    bits = np.where(mask, pk[:, _VALUE_AT:_POLICY_AT, None], np.uint32(0)).astype(np.uint32)
    rec = np.zeros(n, dtype=_RECORD)
    rec["obs"] = bits.reshape(n, OBS_SIZE).view(np.float32)
    rec["policy"] = pk[:, _POLICY_AT + 0].view(np.int32).astype(np.int64)
    rec["value"] = pk[:, _POLICY_AT + 1].view(np.int32).astype(np.int64)
    rec["score"] = pk[:, _POLICY_AT + 2].view(np.float32)
    return rec


def mirror_action(a) -> np.ndarray:
    """The spatial action index ``square * 139 + slot`` of the left-right reflected move (int64, any shape): the square's
    file reversed; sliding slots (``promote * 64 + dir * 8 + dist - 1``, ``dir`` clockwise from north) ``dir -> (8 - dir) % 8``;
    knight slots ``128 + 2 * side + promote`` with the side swapped; drop slots 132..138 unchanged.  An involution."""
    a = np.asarray(a, dtype=np.int64)
    if a.size and (a.min() < 0 or a.max() >= NUM_ACTIONS):
        raise ValueError(f"action indices must lie in [0, {NUM_ACTIONS})")
    square, slot = np.divmod(a, 139)
    square = square + 8 - 2 * (square % 9)
    sliding = (slot & 64) | (((8 - ((slot & 63) >> 3)) & 7) << 3) | (slot & 7)
    slot = np.where(slot < 128, sliding, np.where(slot < 132, slot ^ 2, slot))
    return square * 139 + slot


def mirror_records(records) -> np.ndarray:
    """Shard records of the reflected positions: every plane with its file axis reversed, the policy through
    ``mirror_action``, value and score as they are (``ka_sl_gather_aug`` mode 1 in numpy)."""
    rec = _as_records(records)
    out = rec.copy()
    out["obs"] = rec["obs"].reshape(len(rec), _CHANNELS, 9, 9)[:, :, :, ::-1].reshape(len(rec), OBS_SIZE)
    out["policy"] = mirror_action(rec["policy"])
    return out


def _mix64(x: np.ndarray) -> np.ndarray:
    """The splitmix64 finaliser over uint64 arrays (wrapping arithmetic), ``ka_mix64`` of csrc/common.h."""
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def sl_mirror_draw(seed: int, epoch: int, indices) -> np.ndarray:
    """Which positions ``ka_sl_gather_aug`` reflects in mode 2 (bool, the shape of ``indices``): the top bit of
    ``h = mix(seed ^ mix(((epoch << 32) | index) + 0x6D6972726F72))`` (include/keisei_amd.h), a function of
    (seed, epoch, position) alone."""
    if not 0 <= int(epoch) <= _INT_MAX:
        raise ValueError(f"epoch must lie in [0, 2^31), got {epoch}")
    with np.errstate(over="ignore"):
        i = np.asarray(indices).astype(np.int64).astype(np.uint64) & np.uint64(0xFFFFFFFF)
        key = ((np.uint64(int(epoch)) << np.uint64(32)) | i) + np.uint64(_MIRROR_SALT)
        h = _mix64(np.uint64(int(seed) & _M64) ^ _mix64(key))
    return (h >> np.uint64(63)).astype(bool)


def visit_weights(words) -> np.ndarray:
    """The policy target of visit words ``(..., 8)`` (``action | visits << 16``, visits 0 = unused) as ``ka_sl_gather_visits``
    forms it: float32 ``w_k = (float)N_k / (float)sum N``, one IEEE division, 0 in the unused slots and in a row without
    a used slot."""
    n = (np.asarray(words).astype(np.uint32, copy=False) >> np.uint32(16)).astype(np.float32)
    total = n.sum(axis=-1, keepdims=True, dtype=np.float32)          # integers below 2^24: exact in any order
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n > 0, n / total, np.float32(0)).astype(np.float32)


def mirror_visit_words(words) -> np.ndarray:
    """Visit words of the reflected position: every used slot's action through ``mirror_action``, the visits and the
    unused slots as they are (``ka_sl_gather_visits`` mode 1 on the words).  An involution."""
    w = np.asarray(words).astype(np.uint32, copy=False)
    used = (w >> np.uint32(16)) > 0
    act = np.where(used, w & np.uint32(0xFFFF), 0).astype(np.int64)
    return np.where(used, (w & np.uint32(0xFFFF0000)) | mirror_action(act).astype(np.uint32), w).astype(np.uint32)


def _refuse_mixing(n: int, has_visits: bool, adds_visits: bool, how: str) -> None:
    """A dataset has visit rows for every position or for none."""
    if has_visits and not adds_visits:
        raise ValueError(f"this dataset holds visit rows: {how} would add positions without them (a dataset has visit rows "
                         "for every position or for none)")
    if adds_visits and not has_visits and n > 0:
        raise ValueError(f"this dataset holds {n} positions without visit rows: {how} with visits would mix the two (a "
                         "dataset has visit rows for every position or for none)")


# ---------------------------------------------------------------------------------------------- the device dataset
def _require_library() -> None:
    words = _lib.query("ka_sl_packed_words")                    # raises KeiseiHipError without the library
    if words != PACKED_WORDS:
        raise _lib.KeiseiHipError(f"libkeisei_amd.so packs a position into {words} words, keisei_amd.sl.device_dataset "
                                  f"into {PACKED_WORDS}: rebuild the library")


def _fresh_flags(rows: int, device) -> torch.Tensor:
    return torch.tensor([0, _INT_MAX, 0, _INT_MAX], dtype=torch.int32).repeat(rows, 1).to(device)


class DeviceSLDataset:
    """Positions packed in device memory, in the order they were added.  ``read_batch`` / ``gather`` decode rows."""

    def __init__(self, device=None) -> None:
        _require_library()
        if not torch.cuda.is_available():
            raise _lib.KeiseiHipError("DeviceSLDataset needs a GPU: the dataset lives in device memory")
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise ValueError(f"DeviceSLDataset lives on a GPU, got device {dev}")
        self._device = torch.device("cuda", torch.cuda.current_device() if dev.index is None else dev.index)
        self._packed = torch.empty(0, PACKED_WORDS, dtype=torch.int32, device=self._device)
        self._visits: Optional[torch.Tensor] = None              # int32 (capacity, 8) / (capacity, 4) beside the packed rows:
        self._info: Optional[torch.Tensor] = None                # for every position or for none
        self._n = 0
        self._read_only = False                                  # a view(): rows of another dataset's memory
        # flags of the pack launches not read yet: (index of the launch's first position, int32[4] on the device)
        self._unread: List[Tuple[int, torch.Tensor]] = []

    # ------------------------------------------------------------------ properties
    def __len__(self) -> int:
        return self._n

    @property
    def device(self) -> torch.device:
        return self._device

    @property
    def nbytes(self) -> int:
        """Device bytes the positions occupy (the allocation may be larger while the dataset grows)."""
        return self._n * PACKED_BYTES

    @property
    def packed(self) -> torch.Tensor:
        """The packed rows, int32 ``(len, 204)``: a view of the dataset's memory."""
        return self._packed[:self._n]

    @property
    def visits(self) -> Optional[torch.Tensor]:
        """The visit rows, int32 ``(len, 8)`` (``action | visits << 16`` per slot, visits 0 = unused): a view of the
        dataset's memory; None for a dataset without them."""
        return None if self._visits is None else self._visits[:self._n]

    @property
    def info(self) -> Optional[torch.Tensor]:
        """The info rows, int32 ``(len, 4)`` (``model | mover << 16``, index of the move in its game, env, game number);
        None for a dataset without visit rows."""
        return None if self._info is None else self._info[:self._n]

    # ------------------------------------------------------------------ filling
    def _reserve(self, total: int) -> None:
        """Room for ``total`` positions; growth doubles, the rows keep their order."""
        cap = self._packed.shape[0]
        if total <= cap:
            return
        with torch.cuda.device(self._device):
            grown = torch.empty(max(total, 2 * cap, 1024), PACKED_WORDS, dtype=torch.int32, device=self._device)
            grown[:self._n].copy_(self._packed[:self._n])
            if self._visits is not None:
                for name, width in (("_visits", VISIT_SLOTS), ("_info", INFO_WORDS)):
                    side = torch.zeros(grown.shape[0], width, dtype=torch.int32, device=self._device)
                    side[:self._n].copy_(getattr(self, name)[:self._n])
                    setattr(self, name, side)
        self._packed = grown

    def _pack(self, raw: torch.Tensor, src_rows: Optional[torch.Tensor], count: int, flags: torch.Tensor) -> None:
        """Queue ``ka_sl_pack`` of ``count`` records onto the end (room reserved by the caller)."""
        with torch.cuda.device(self._device):
            _lib.call("ka_sl_pack", raw, src_rows, count, self._packed[self._n:], flags, _lib.stream_ptr(self._device))
        self._unread.append((self._n, flags))
        self._n += count

    def append_raw(self, raw_device_bytes: torch.Tensor, src_rows) -> None:
        """Pack the records ``src_rows`` (row numbers, in the order they are to be appended) of a device buffer of
        16 220-byte records onto the end.  Nothing is read back: ``check()`` reports what could not be packed."""
        if self._read_only:
            raise ValueError("this dataset is a view of another one's memory and cannot grow: append to its parent")
        _refuse_mixing(self._n, self._visits is not None, False, "append_raw")
        raw = raw_device_bytes
        if raw.dtype != torch.uint8 or not raw.is_contiguous() or raw.device != self._device or raw.numel() % RECORD_SIZE:
            raise ValueError(f"raw_device_bytes must be a contiguous uint8 tensor of whole {RECORD_SIZE}-byte records "
                             f"on {self._device}")
        rows = np.ascontiguousarray(src_rows.cpu().numpy() if isinstance(src_rows, torch.Tensor) else src_rows,
                                    dtype=np.int64).reshape(-1)
        total = raw.numel() // RECORD_SIZE
        if rows.size and (rows.min() < 0 or rows.max() >= total):
            bad = int(rows[(rows < 0) | (rows >= total)][0])
            raise IndexError(f"source row {bad} out of range for a buffer of {total} records")
        if rows.size == 0:
            return
        self._reserve(self._n + rows.size)
        self._pack(raw, torch.from_numpy(rows).to(self._device), int(rows.size), _fresh_flags(1, self._device)[0])

    def append_packed(self, packed: torch.Tensor, visits: Optional[torch.Tensor] = None,
                      info: Optional[torch.Tensor] = None) -> None:
        """Append positions that are already packed -- ``packed`` int32 ``(m, 204)`` on the dataset's device -- device to
        device; with ``visits`` int32 ``(m, 8)`` (and ``info`` int32 ``(m, 4)``, zeros when left out) the dataset holds visit
        rows.  A dataset has them for every position or for none: mixing raises.  The rows are validated on the device
        and nothing is read back: ``check()`` reports the lowest row whose policy lies outside [0, 11259), whose value
        outside {0, 1, 2}, that has a used visit word naming no action, or that has no used visit word at all."""
        if self._read_only:
            raise ValueError("this dataset is a view of another one's memory and cannot grow: append to its parent")
        _refuse_mixing(self._n, self._visits is not None, visits is not None, "append_packed")
        if info is not None and visits is None:
            raise ValueError("info rows come with visit rows: append_packed(info=) needs visits=")
        m = int(packed.shape[0]) if packed.dim() == 2 else -1
        for name, t, width in (("packed", packed, PACKED_WORDS), ("visits", visits, VISIT_SLOTS), ("info", info, INFO_WORDS)):
            if t is not None and (t.dtype != torch.int32 or tuple(t.shape) != (m, width) or t.device != self._device
                                  or not t.is_contiguous()):
                raise ValueError(f"{name} must be a contiguous int32 tensor ({max(m, 0)}, {width}) on {self._device}")
        if m == 0:
            return
        self._reserve(self._n + m)
        with torch.cuda.device(self._device):
            if visits is not None and self._visits is None:
                cap = self._packed.shape[0]
                self._visits = torch.zeros(cap, VISIT_SLOTS, dtype=torch.int32, device=self._device)
                self._info = torch.zeros(cap, INFO_WORDS, dtype=torch.int32, device=self._device)
            lo = self._n
            self._packed[lo:lo + m].copy_(packed)
            policy, value = packed[:, _POLICY_AT], packed[:, _POLICY_AT + 1]
            bad = (policy < 0) | (policy >= NUM_ACTIONS) | (value < 0) | (value > 2)
            if visits is not None:
                self._visits[lo:lo + m].copy_(visits)
                if info is None:
                    self._info[lo:lo + m].zero_()
                else:
                    self._info[lo:lo + m].copy_(info)
                used = (visits >> 16) != 0                       # (an arithmetic shift: a count with bit 15 set is used too)
                bad |= (used & ((visits & 0xFFFF) >= NUM_ACTIONS)).any(1) | ~used.any(1)
            at = torch.where(bad, torch.arange(m, device=self._device), torch.full((), _INT_MAX, device=self._device)).min()
            zero = torch.zeros((), dtype=torch.int64, device=self._device)
            flags = torch.stack([zero, zero + _INT_MAX, bad.sum(), at]).to(torch.int32)
        self._unread.append((lo, flags))
        self._n += m

    def check(self, describe: Optional[Callable[[int, bool], None]] = None) -> None:
        """Read the flags of every pack launch since the last check -- one read -- and raise ``ValueError`` for the
        lowest position that has an invalid target or cannot be held packed.  ``describe(index, bad_target)`` may raise a
        message of its own first (``from_shards`` names the shard)."""
        if not self._unread:
            return
        starts = [s for s, _ in self._unread]
        host = torch.stack([f for _, f in self._unread]).cpu().numpy()
        self._unread = []
        faults = []                                              # (index, 0 for a bad target / 1 for unpackable)
        for start, (unpackable, at_u, bad_target, at_t) in zip(starts, host.tolist()):
            if bad_target:
                faults.append((start + at_t, 0))
            if unpackable:
                faults.append((start + at_u, 1))
        if not faults:
            return
        index, kind = min(faults)
        if describe is not None:
            describe(index, kind == 0)
        if kind == 0:
            policy, value = self._packed[index, _POLICY_AT:_POLICY_AT + 2].cpu().tolist()
            more = ""
            if self._visits is not None:
                words = [f"{w & 0xFFFFFFFF:#x}" for w in self._visits[index].cpu().tolist()]
                more = (f"; its visit words {words} must hold a used slot, and every used slot (visits << 16 != 0) an action "
                        f"in [0, {NUM_ACTIONS})")
            raise ValueError(f"Invalid targets (policy_target={policy}, value_target={value} as stored) at index {index}: "
                             f"policy must be in [0, {NUM_ACTIONS}), value 0 (W), 1 (D), or 2 (L){more}")
        raise ValueError(f"Unpackable observation at index {index}: {_UNPACKABLE}")

    @classmethod
    def from_shards(cls, data_dir, *, device=None, chunk_records: int = 8192,
                    allow_placeholder: bool = False) -> "DeviceSLDataset":
        """The positions of a shard directory, in ``SLDataset``'s order (which also refuses placeholder data and warns
        about the files).  The maps stream in chunks of ``chunk_records`` -- a chunk may straddle files -- through two pinned
        staging buffers and a copy stream; each chunk is packed on arrival into its place in one device allocation."""
        if chunk_records < 1:
            raise ValueError(f"chunk_records must be >= 1, got {chunk_records}")
        source = SLDataset(Path(data_dir), allow_placeholder=allow_placeholder)
        self = cls(device)
        dev, n = self._device, len(source)
        if n == 0:
            return self
        if n > _INT_MAX:
            raise ValueError(f"{n} positions: a device dataset holds at most {_INT_MAX}")
        chunk = min(int(chunk_records), n)
        chunks = (n + chunk - 1) // chunk
        needed = n * PACKED_BYTES + 2 * chunk * RECORD_SIZE
        free = torch.cuda.mem_get_info(dev)[0]
        if needed > free:
            raise ValueError(f"The dataset in {data_dir} does not fit on {dev}: {n} positions need {needed} bytes "
                             f"({n * PACKED_BYTES} packed + {2 * chunk * RECORD_SIZE} staging), {free} bytes are free")
        with torch.cuda.device(dev):
            self._packed = torch.empty(n, PACKED_WORDS, dtype=torch.int32, device=dev)
            flags = _fresh_flags(chunks, dev)
            pinned = [torch.empty(chunk * RECORD_SIZE, dtype=torch.uint8).pin_memory() for _ in range(2)]
            staged = [torch.empty(chunk * RECORD_SIZE, dtype=torch.uint8, device=dev) for _ in range(2)]
            packed_ev: List[Optional[torch.cuda.Event]] = [None, None]
            main, copy_stream = torch.cuda.current_stream(dev), torch.cuda.Stream(dev)
            shard, local = 0, 0
            for k in range(chunks):
                slot, count = k & 1, min(chunk, n - k * chunk)
                if packed_ev[slot] is not None:
                    packed_ev[slot].synchronize()                # chunk k - 2 has left both buffers of this slot
                host = pinned[slot].numpy()[:count * RECORD_SIZE].view(_RECORD)
                filled = 0
                while filled < count:
                    take = min(count - filled, source.shards[shard][1] - local)
                    host[filled:filled + take] = source._records(shard)[local:local + take]
                    filled, local = filled + take, local + take
                    if local == source.shards[shard][1]:
                        shard, local = shard + 1, 0
                with torch.cuda.stream(copy_stream):
                    staged[slot][:count * RECORD_SIZE].copy_(pinned[slot][:count * RECORD_SIZE], non_blocking=True)
                    arrived = torch.cuda.Event()
                    arrived.record(copy_stream)
                main.wait_event(arrived)
                self._pack(staged[slot], None, count, flags[k])
                packed_ev[slot] = torch.cuda.Event()
                packed_ev[slot].record(main)

        def describe(index: int, bad_target: bool) -> None:
            at, where = source._locate(index)
            rec = source._records(at)[where]
            if bad_target:
                source._check_targets(int(rec["policy"]), int(rec["value"]), index, at, where)
            raise ValueError(f"Unpackable observation at index {index} (shard={source.shards[at][0].name}, local={where}): "
                             f"{_UNPACKABLE}")

        self.check(describe)                                     # the one read of the flags (it also ends the copies)
        source.clear_cache()
        return self

    def view(self, start: int, stop: int) -> "DeviceSLDataset":
        """The positions ``[start, stop)`` as a dataset over the SAME device memory: no copy, read-only (``append_raw``
        raises).  It covers the rows as they lie when it is taken: a parent that grows past its allocation afterwards
        moves on to new memory and the view keeps the old.  Positions not checked yet stay the parent's to ``check()``."""
        start, stop = int(start), int(stop)
        if not 0 <= start <= stop <= self._n:
            raise IndexError(f"view [{start}, {stop}) out of range for dataset with {self._n} positions")
        part = DeviceSLDataset(self._device)
        part._packed = self._packed[start:stop]
        if self._visits is not None:
            part._visits, part._info = self._visits[start:stop], self._info[start:stop]
        part._n = stop - start
        part._read_only = True
        return part

    # ------------------------------------------------------------------ reading
    def gather(self, idx: torch.Tensor, flag: torch.Tensor, *, mirror: int = MIRROR_NONE, seed: int = 0, epoch: int = 0,
               visit_targets: bool = False) -> dict:
        """The batch of the int64 device tensor ``idx`` as fresh device tensors, keys / dtypes / shapes of
        ``SLDataset.read_batch``: one launch, no host work.  An index outside the dataset adds 1 to ``flag`` (int32[1] on
        the device) and gives a zero row.  ``mirror``: 0 the rows as stored, 1 every row reflected left to right, 2 the rows
        ``sl_mirror_draw(seed, epoch, idx)`` names.  ``visit_targets=True`` (a dataset with visit rows) adds
        ``visit_actions`` (int32 ``(B, 8)``, -1 = unused) and ``visit_weights`` (fp32 ``(B, 8)``, ``visit_weights`` of the rows)
        from a second launch, ``ka_sl_gather_visits``, which reflects the actions of the rows the first one reflects."""
        if visit_targets and self._visits is None:
            raise ValueError("visit_targets=True needs a dataset with visit rows (append_packed(..., visits=), or the "
                             "dataset SearchSamples.drain() gives)")
        if idx.dtype != torch.int64 or idx.dim() != 1 or idx.device != self._device or not idx.is_contiguous():
            raise ValueError(f"idx must be a contiguous 1-d int64 tensor on {self._device}")
        if mirror not in (MIRROR_NONE, MIRROR_ALL, MIRROR_DRAWN):
            raise ValueError(f"mirror must be 0 (off), 1 (every row) or 2 (drawn per row), got {mirror!r}")
        if not 0 <= int(epoch) <= _INT_MAX:
            raise ValueError(f"epoch must lie in [0, 2^31), got {epoch}")
        B, dev = idx.shape[0], self._device
        with torch.cuda.device(dev):
            out = {"observation": torch.empty(B, _CHANNELS, 9, 9, dtype=torch.float32, device=dev),
                   "policy_target": torch.empty(B, dtype=torch.int64, device=dev),
                   "value_target": torch.empty(B, dtype=torch.int64, device=dev),
                   "score_target": torch.empty(B, dtype=torch.float32, device=dev)}
            if B and mirror == MIRROR_NONE:
                _lib.call("ka_sl_gather", self._packed, self._n, idx, B, out["observation"], out["policy_target"],
                          out["value_target"], out["score_target"], flag, _lib.stream_ptr(dev))
            elif B:
                seed64 = int(seed) & _M64                        # the C ABI takes the 64 bits as a signed long long
                _lib.call("ka_sl_gather_aug", self._packed, self._n, idx, B, out["observation"], out["policy_target"],
                          out["value_target"], out["score_target"], flag, int(mirror),
                          seed64 - (1 << 64) if seed64 >> 63 else seed64, int(epoch), _lib.stream_ptr(dev))
            if visit_targets:
                out["visit_actions"] = torch.empty(B, VISIT_SLOTS, dtype=torch.int32, device=dev)
                out["visit_weights"] = torch.empty(B, VISIT_SLOTS, dtype=torch.float32, device=dev)
                if B:
                    seed64 = int(seed) & _M64
                    _lib.call("ka_sl_gather_visits", self._visits, self._n, idx, B, int(mirror),
                              seed64 - (1 << 64) if seed64 >> 63 else seed64, int(epoch), out["visit_actions"],
                              out["visit_weights"], flag, _lib.stream_ptr(dev))
        return out

    def read_batch(self, indices) -> dict:
        """``SLDataset.read_batch(indices)`` as device tensors.  (The range check on the host is this convenience
        method's; the training epoch reads the kernel's flag once instead.)"""
        idx = np.asarray(indices.cpu() if isinstance(indices, torch.Tensor) else indices, dtype=np.int64).reshape(-1)
        if idx.size and (idx.min() < 0 or idx.max() >= self._n):
            bad = int(idx[(idx < 0) | (idx >= self._n)][0])
            raise IndexError(f"index {bad} out of range for dataset with {self._n} positions")
        return self.gather(torch.from_numpy(np.ascontiguousarray(idx)).to(self._device),
                           torch.zeros(1, dtype=torch.int32, device=self._device))
