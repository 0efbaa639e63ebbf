"""DynamicTrainer: small PPO updates of the league's Dynamic entries from match rollouts (mirror of
keisei/training/dynamic_trainer.py:25-418: same constructor, method names, return values, counters, logging levels and
error policy).

Three execution paths share the host policy:

* **cpu**: CPU tensors, any ``nn.Module``: the reference's statement sequence on tensor ops (dynamic_trainer.py:288-378).
* **fused**: an ``SEResNetModel`` on a GPU: ``ka_dynamic_targets`` makes the W/D/L labels and the advantages, the
  ``old_log_probs`` come from eval-mode forwards of the engine and ``ka_policy_loss`` (its guard flags included), and
  every epoch is one whole-batch step of ``KataGoPPOAlgorithm``'s fused machinery (gather + forward + ``ka_policy_loss`` +
  ``ka_value_loss`` + backward + ``ka_clip_adam_step``) with lambda_policy = lambda_value = 1, no score term, no entropy
  term, clip 0.2.  fp32 unless ``use_amp=True``.
* **generic**: any other model on a GPU: the cpu sequence on device tensors, logged once, refused under
  ``KEISEI_AMD_STRICT=1`` (as ``KataGoPPOAlgorithm.update`` does).

``MatchRollout`` holds either the reference's ``(steps, envs, ...)`` tensors with bool ``legal_masks`` or the flat
``(rows, ...)`` device tensors ``MatchArena(collect=True)`` returns, whose masks are packed (``legal_mask_bits``).

``attach_group(group, index_of)`` closes the league loop on the device: an attached entry's update trains the group's own
resident module, leaves it in eval mode and refreshes the group, so the next ``MatchArena`` round plays the new weights.

The store and the config are duck-typed: ``load_opponent``, ``load_optimizer``, ``save_weights``, ``save_optimizer``,
``increment_update_count``, ``get_entry``; and the ``DynamicConfig`` fields read below.
"""
from __future__ import annotations

import logging
import os
import threading
import time
from collections import deque
from dataclasses import dataclass
from typing import Any, Dict, Optional

import torch
import torch.nn.functional as F

from keisei_amd import _lib
from keisei_amd.training.katago_ppo import (KataGoPPOAlgorithm, KataGoPPOParams, ppo_clip_loss,
                                            wdl_cross_entropy_loss)
from keisei_amd.training.models.se_resnet import SEResNetModel

logger = logging.getLogger(__name__)

CLIP_EPSILON = 0.2                     # dynamic_trainer.py:360-362
_EVAL_CHUNK = 2048                     # rows per eval-mode forward of the old_log_probs pass (no tensor couples two boards)


@dataclass
class MatchRollout:
    """Replay data of one league match (dynamic_trainer.py:25-38).

    Reference layout: ``(steps, num_envs, ...)`` CPU tensors, ``legal_masks`` bool ``(steps, num_envs, action_space)``.
    Arena layout: flat ``(rows, ...)`` tensors on the arena's device, ``legal_masks`` None and ``legal_mask_bits`` the
    packed int32 rows ``(rows, ceil(action_space / 32))`` (bit j of word w = action 32 w + j)."""

    observations: torch.Tensor
    actions: torch.Tensor
    rewards: torch.Tensor
    dones: torch.Tensor
    legal_masks: Optional[torch.Tensor]
    perspective: torch.Tensor            # 0 = player A, 1 = player B
    legal_mask_bits: Optional[torch.Tensor] = None


def unpack_mask_bits(bits: torch.Tensor, action_space: int) -> torch.Tensor:
    """Packed int32 rows (n, words) -> bool rows (n, action_space), on the tensor's own device (plain tensor ops)."""
    j = torch.arange(action_space, device=bits.device)
    return ((bits[:, j // 32] >> (j % 32)) & 1).bool()


def pack_mask_bits(masks: torch.Tensor) -> torch.Tensor:
    """bool rows (n, A) -> packed int32 rows (n, ceil(A / 32)), the inverse of ``unpack_mask_bits``."""
    n, A = masks.shape
    words = (A + 31) // 32
    padded = torch.zeros(n, words * 32, dtype=torch.int64, device=masks.device)
    padded[:, :A] = masks.to(torch.int64)
    w = (padded.view(n, words, 32) << torch.arange(32, device=masks.device)).sum(dim=-1)
    return torch.where(w >= 2 ** 31, w - 2 ** 32, w).to(torch.int32)


class DynamicTrainer:
    """Small PPO updates for Dynamic entries from league match data (dynamic_trainer.py:41-418).

    ``record_match``, ``should_update``, ``is_rate_limited`` and ``update`` are called from the tournament thread;
    ``_update_lock`` serialises ``update`` calls so no other thread sees a half-updated model."""

    def __init__(self, store: Any, config: Any, learner_lr: float, *, use_amp: bool = False) -> None:
        self.store = store
        self.config = config
        self.learner_lr = learner_lr
        self.use_amp = bool(use_amp)                 # extension: bf16 autocast on the fused path (the reference trains fp32)

        self._match_counts: Dict[int, int] = {}
        self._total_matches: Dict[int, int] = {}
        self._update_timestamps: list = []
        self._optimizers: Dict[int, torch.optim.Adam] = {}
        self._disabled_entries: set = set()
        self._rollout_buffers: Dict[int, deque] = {}
        self._error_counts: Dict[int, int] = {}
        self._globally_disabled: bool = False
        self._global_error_timestamps: list = []
        self._update_lock = threading.Lock()

        self.last_update_path: Optional[str] = None  # "fused" | "generic" | "cpu"
        self.last_old_log_probs: Optional[torch.Tensor] = None
        self._group = None
        self._group_index: Dict[int, int] = {}
        self._warned_generic: set = set()

    # ------------------------------------------------------------------ closing the loop
    def attach_group(self, group, index_of: Dict[int, int]) -> None:
        """Train attached entries in place: ``index_of[entry_id]`` is the entry's model index in ``group`` (an
        ``SEResNetGroup``, typically the one a ``MatchArena`` plays with)."""
        for entry_id, k in index_of.items():
            if not 0 <= int(k) < len(group):
                raise ValueError(f"entry {entry_id}: model index {k} outside the group's [0, {len(group)})")
        self._group = group
        self._group_index = {eid: int(k) for eid, k in index_of.items()}

    # ------------------------------------------------------------------ record & query
    def record_match(self, entry_id: int, rollout: MatchRollout, side: int) -> None:
        if entry_id in self._disabled_entries:                                        # :80-81
            return
        if entry_id not in self._rollout_buffers:
            self._rollout_buffers[entry_id] = deque(maxlen=self.config.max_buffer_depth)   # :82-83
        self._rollout_buffers[entry_id].append((rollout, side))
        self._match_counts[entry_id] = self._match_counts.get(entry_id, 0) + 1

    def should_update(self, entry_id: int) -> bool:
        if self._globally_disabled or entry_id in self._disabled_entries:             # :89-92
            return False
        return self._match_counts.get(entry_id, 0) >= self.config.update_every_matches

    def is_rate_limited(self) -> bool:
        """Too many updates in the last 60 seconds (:95-105; a timestamp exactly 60 s old still counts)."""
        cutoff = time.monotonic() - 60.0
        self._update_timestamps = [t for t in self._update_timestamps if t >= cutoff]
        return len(self._update_timestamps) >= self.config.max_updates_per_minute

    @property
    def is_globally_disabled(self) -> bool:
        return self._globally_disabled

    def is_gpu_backpressured(self, device: str) -> bool:
        """Reserved GPU memory at or above ``gpu_memory_backpressure`` of the card (:112-129)."""
        if not device.startswith("cuda") or not torch.cuda.is_available():
            return False
        dev = torch.device(device)
        total = torch.cuda.get_device_properties(dev).total_memory
        if total == 0:
            return False
        used = torch.cuda.memory_reserved(dev) / total
        if used >= self.config.gpu_memory_backpressure:
            logger.info("GPU backpressure: %.1f%% memory reserved (threshold %.0f%%)", used * 100,
                        self.config.gpu_memory_backpressure * 100)
            return True
        return False

    def _check_global_disable(self) -> None:
        """Errors of all entries inside the window against the global threshold (:131-150)."""
        cutoff = time.monotonic() - self.config.global_error_window_seconds
        self._global_error_timestamps = [t for t in self._global_error_timestamps if t >= cutoff]
        if len(self._global_error_timestamps) >= self.config.global_error_threshold:
            self._globally_disabled = True
            logger.error("DynamicTrainer globally disabled: %d errors in %.0fs window (threshold %d). "
                         "All Dynamic training stopped.", len(self._global_error_timestamps),
                         self.config.global_error_window_seconds, self.config.global_error_threshold)

    def get_update_stats(self, entry_id: int):
        entry = self.store.get_entry(entry_id)
        if entry is None:
            return (0, None)
        return (entry.update_count, entry.last_train_at)

    # ------------------------------------------------------------------ batch
    def _prepare_batch(self, entry_id: int, device: str):
        """Concatenate the entry's rollouts, each filtered by ``perspective == side`` (:163-200).  Returns
        ``(obs, actions, rewards, dones, masks)`` on ``device``; ``masks`` are bool rows, or packed int32 rows when every
        buffered rollout is packed (mixed buffers are unpacked)."""
        buffers = self._rollout_buffers.get(entry_id, [])
        cols = ([], [], [], [], [])
        packed = []
        for rollout, side in buffers:
            assert rollout.perspective.shape == rollout.actions.shape, (
                f"perspective shape {rollout.perspective.shape} must match actions shape {rollout.actions.shape}")
            keep = rollout.perspective == side
            if rollout.legal_masks is not None:
                masks, is_packed = rollout.legal_masks[keep], False
            elif rollout.legal_mask_bits is not None:
                masks, is_packed = rollout.legal_mask_bits[keep], True
            else:
                raise ValueError("MatchRollout needs legal_masks or legal_mask_bits")
            for out, t in zip(cols, (rollout.observations[keep], rollout.actions[keep], rollout.rewards[keep],
                                     rollout.dones[keep], masks)):
                out.append(t)
            packed.append(is_packed)
        if not cols[0]:
            empty = torch.zeros(0)                   # the caller only looks at shape[0] (:188-192)
            return empty, empty, empty, empty, empty
        if any(packed) and not all(packed):
            A = next(m.shape[-1] for m, p in zip(cols[4], packed) if not p)
            cols[4][:] = [unpack_mask_bits(m, A) if p else m for m, p in zip(cols[4], packed)]
        return tuple(torch.cat([t.to(device) for t in c]) for c in cols)

    # ------------------------------------------------------------------ optimiser
    def _get_or_create_optimizer(self, entry_id: int, model: torch.nn.Module) -> torch.optim.Adam:
        """A fresh Adam on the model's parameters at ``learner_lr * lr_scale``, carrying over the cached state of the
        entry's last successful update, or else the state the store holds (:202-245)."""
        optimizer = torch.optim.Adam(model.parameters(), lr=self.learner_lr * self.config.lr_scale)
        cached = self._optimizers.get(entry_id)
        saved = cached.state_dict() if cached is not None else self.store.load_optimizer(entry_id)
        if saved is None:
            return optimizer
        try:
            optimizer.load_state_dict(saved)
            device = next(model.parameters()).device
            for state in optimizer.state.values():
                for k, v in state.items():
                    if isinstance(v, torch.Tensor):
                        state[k] = v.to(device)
        except (ValueError, RuntimeError):
            if cached is not None:
                logger.warning("Optimizer state mismatch for entry %d, resetting momentum", entry_id)
            else:
                logger.warning("Failed to load optimizer state for entry %d, starting fresh", entry_id)
        return optimizer

    # ------------------------------------------------------------------ update
    def update(self, entry: Any, device: str) -> bool:
        """One small PPO update of ``entry`` from its buffered rollouts.  True on success, False when an error was
        caught and handled; raises when ``config.disable_on_error`` is false (:247-257)."""
        with self._update_lock:
            return self._update_guarded(entry, device)

    def _update_guarded(self, entry: Any, device: str) -> bool:
        try:
            return self._update_inner(entry, device)
        except Exception:
            if not self.config.disable_on_error:
                raise
            cfg = self.config
            self._match_counts[entry.id] = 0                                          # :266-268 stale data is dropped
            self._rollout_buffers[entry.id] = deque(maxlen=cfg.max_buffer_depth)
            self._error_counts[entry.id] = self._error_counts.get(entry.id, 0) + 1
            self._global_error_timestamps.append(time.monotonic())
            logger.warning("DynamicTrainer update failed for entry %d (error %d/%d)", entry.id,
                           self._error_counts[entry.id], cfg.max_consecutive_errors, exc_info=True)
            if self._error_counts[entry.id] >= cfg.max_consecutive_errors:
                self._disabled_entries.add(entry.id)
                logger.error("DynamicTrainer disabled entry %d after %d consecutive errors", entry.id,
                             cfg.max_consecutive_errors)
            self._check_global_disable()
            return False

    def _update_inner(self, entry: Any, device: str) -> bool:
        attached = self._group is not None and entry.id in self._group_index
        if attached:
            model = self._group.models[self._group_index[entry.id]]
            model.eval()
        else:
            model = self.store.load_opponent(entry, device)                           # eval mode (:290-293)
        try:
            batch = self._prepare_batch(entry.id, device)
            if batch[0].shape[0] == 0:
                return False                                                          # :300-301
            dev = torch.device(device)
            if dev.type != "cuda":
                self.last_update_path = "cpu"
                optimizer = self._train_generic(entry.id, model, batch, device)
            elif isinstance(model, SEResNetModel):
                self.last_update_path = "fused"
                with torch.cuda.device(dev):
                    optimizer = self._train_fused(entry.id, model, batch, dev)
            else:
                why = f"model is {type(model).__name__}, not SEResNetModel"
                if os.environ.get("KEISEI_AMD_STRICT", "0") == "1":
                    raise _lib.KeiseiHipError(f"update() cannot take the fused HIP step: {why} (KEISEI_AMD_STRICT=1)")
                if why not in self._warned_generic:
                    self._warned_generic.add(why)
                    logger.warning("update() on %s runs the generic torch-op step, not the fused HIP step: %s", device, why)
                self.last_update_path = "generic"
                optimizer = self._train_generic(entry.id, model, batch, device)
            if attached:
                model.eval()
                self._group.refresh()                                                 # the next round plays the new weights
        finally:
            if attached:
                model.eval()

        self.store.save_weights(entry.id, model.state_dict())                         # :380-381

        # Weights are committed: what fails below is bookkeeping, not training (:383-410)
        try:
            for state in optimizer.state.values():
                for k, v in state.items():
                    if isinstance(v, torch.Tensor):
                        state[k] = v.cpu()
            self._total_matches[entry.id] = self._total_matches.get(entry.id, 0) + self._match_counts.get(entry.id, 0)
            if self._total_matches[entry.id] >= self.config.checkpoint_flush_every:
                self.store.save_optimizer(entry.id, optimizer.state_dict())
                self._total_matches[entry.id] %= self.config.checkpoint_flush_every
            self.store.increment_update_count(entry.id)
        except Exception:
            logger.warning("Post-checkpoint bookkeeping failed for entry %d (weights were saved successfully)", entry.id,
                           exc_info=True)

        self._match_counts[entry.id] = 0
        self._rollout_buffers[entry.id] = deque(maxlen=self.config.max_buffer_depth)
        self._update_timestamps.append(time.monotonic())
        self._error_counts[entry.id] = 0
        self._optimizers[entry.id] = optimizer                                        # kept on success only
        return True

    # ---- cpu / generic: the reference's statement sequence (:303-378) ---------------------
    def _train_generic(self, entry_id: int, model: torch.nn.Module, batch, device: str) -> torch.optim.Adam:
        obs, actions, rewards, dones, masks = batch
        n = obs.shape[0]
        if masks.dtype != torch.bool:
            if masks.dtype == torch.int32 and masks.dim() == 2 and masks.shape[1] < 1024:     # packed rows
                with torch.no_grad():
                    A = model(obs[:1]).policy_logits.reshape(1, -1).shape[1]
                masks = unpack_mask_bits(masks, A)
            else:
                masks = masks.bool()
        cats = torch.full((n,), -1, dtype=torch.long, device=device)
        terminal = dones.bool()
        cats[terminal & (rewards > 0)] = 0           # win  (rewards are literal +-1 / 0: exact comparison)
        cats[terminal & (rewards == 0)] = 1          # draw (truncated games: reward 0)
        cats[terminal & (rewards < 0)] = 2           # loss

        def log_probs_of(out, rows):
            logits = out.policy_logits.reshape(rows.shape[0], -1)
            logp = F.log_softmax(logits.masked_fill(~masks[rows], float("-inf")), dim=-1)
            return logp.gather(1, actions[rows].unsqueeze(1)).squeeze(1)

        with torch.no_grad():                        # eval mode: the running statistics the match was played with
            old_lp = log_probs_of(model(obs), torch.arange(n, device=obs.device))
        self.last_old_log_probs = old_lp.detach()
        model.train()
        optimizer = self._get_or_create_optimizer(entry_id, model)
        for _ in range(self.config.update_epochs_per_batch):
            rows = torch.randperm(n, device=device)
            out = model(obs[rows])
            new_lp = log_probs_of(out, rows)
            advantages = rewards[rows] * dones[rows].float()
            policy_loss = ppo_clip_loss(new_lp, old_lp[rows], advantages, clip_epsilon=CLIP_EPSILON)
            value_loss = wdl_cross_entropy_loss(out.value_logits, cats[rows])
            loss = policy_loss + value_loss          # equal weights, no entropy bonus, no score head (:367-373)
            optimizer.zero_grad()
            loss.backward()
            torch.nn.utils.clip_grad_norm_(model.parameters(), self.config.grad_clip)
            optimizer.step()
        eng = getattr(model, "_hip_engine", None)
        if eng is not None:
            eng.notify_weights_updated()
        return optimizer

    # ---- fused HIP path ---------------------------------------------------------------------
    def _train_fused(self, entry_id: int, model: SEResNetModel, batch, dev: torch.device) -> torch.optim.Adam:
        obs, actions, rewards, dones, masks = batch
        n = obs.shape[0]
        sp = _lib.stream_ptr(dev)
        col = lambda t, dt: t.to(device=dev, dtype=dt).reshape(n).contiguous()  # noqa: E731
        A = SEResNetModel.SPATIAL_ACTION_SPACE
        words = _lib.query("ka_mask_words", A)
        if masks.dtype == torch.int32 and masks.dim() == 2 and masks.shape[1] == words:
            masks, mask_words = masks.contiguous(), words
        else:
            masks, mask_words = masks.to(torch.bool).reshape(n, A).contiguous(), 0
        obs = obs.to(dtype=torch.float32).contiguous()
        actions, rewards, dones = col(actions, torch.int64), col(rewards, torch.float32), col(dones, torch.float32)
        cats = torch.empty(n, dtype=torch.int64, device=dev)
        adv = torch.empty(n, device=dev)
        _lib.call("ka_dynamic_targets", rewards, dones, cats, adv, n, sp)

        saved_amp = (model._amp_enabled, model._amp_dtype, model._amp_device_type)
        params = KataGoPPOParams(learning_rate=self.learner_lr * self.config.lr_scale, clip_epsilon=CLIP_EPSILON,
                                 epochs_per_batch=self.config.update_epochs_per_batch, batch_size=n, lambda_policy=1.0,
                                 lambda_value=1.0, lambda_score=0.0, lambda_entropy=0.0, grad_clip=self.config.grad_clip,
                                 use_amp=self.use_amp)
        try:
            algo = KataGoPPOAlgorithm(params, model)                 # sets the model's autocast mode; owns the fused step
            old_lp = torch.empty(n, device=dev)
            dataset = {"obs": obs, "masks": masks, "mask_words": mask_words, "n_actions": A, "actions": actions,
                       "old_lp": old_lp, "adv": adv, "cats": cats, "score_t": torch.zeros(n, device=dev)}
            algo.optimizer = self._get_or_create_optimizer(entry_id, model)
            if not algo._fused_optimizer_ok():
                raise _lib.KeiseiHipError("Dynamic update: the fused step needs contiguous fp32 parameters")
            fs = algo._fused_begin(dataset, dev, None)
            # old_log_probs: eval-mode forwards in chunks, log-prob gather by ka_policy_loss (no gradient output); an
            # action outside the action space or a row without a legal action sets the flags the optimiser step obeys
            zeros = torch.zeros(n, device=dev)
            scratch = torch.empty(2, min(n, _EVAL_CHUNK), device=dev)
            with torch.no_grad():
                for lo in range(0, n, _EVAL_CHUNK):
                    idx = torch.arange(lo, min(lo + _EVAL_CHUNK, n), device=dev)
                    b = idx.shape[0]
                    out = model(obs, gather_idx=idx)
                    logits = out.policy_logits.reshape(b, A)
                    _lib.call("ka_policy_loss", logits, masks, actions, zeros, zeros, idx, None, old_lp[lo:lo + b],
                              scratch[0, :b], scratch[1, :b], fs["flags"], None, CLIP_EPSILON, 0.0, 0.0, b, A, mask_words, sp)
            self.last_old_log_probs = old_lp
            model.train()
            for _ in range(self.config.update_epochs_per_batch):
                algo._fused_step(fs, torch.randperm(n, device=dev), dev)      # whole batch: BatchNorm statistics over all rows
            algo._fused_end(fs)                                      # the one synchronisation; raises on a guard flag
            return algo.optimizer
        except torch.OutOfMemoryError as e:
            raise RuntimeError(f"Dynamic update: a whole-batch step of {n} rows does not fit the engine's workspace on "
                               f"{dev} (the train-mode step cannot be split: BatchNorm statistics are over the batch)") from e
        finally:
            model._amp_enabled, model._amp_dtype, model._amp_device_type = saved_amp
