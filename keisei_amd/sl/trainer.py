"""Supervised-learning trainer for the KataGo-contract models (API mirror of keisei/sl/trainer.py:19-191).

``SLConfig`` / ``SLTrainer(model, config).train_epoch() -> {"policy_loss", "value_loss", "score_loss"}`` keep the
reference's names, defaults, validation and side effects (Adam, GradScaler, one CosineAnnealingLR tick per epoch that
trained on data).  Two execution paths:

* **fused HIP path** (``SEResNetModel`` on a CUDA/HIP device, fp32 or bf16 AMP): the same forward / backward kernels
  as the PPO update, ``ka_policy_ce`` (cross-entropy over the 11 259 actions + its gradient in one pass over the
  logits) and ``ka_value_loss`` (W/D/L cross-entropy, score MSE, the batch means) instead of the reference's three
  loss ops and their autograd, and the fused GradScaler/clip/Adam launch.  Batches are gathered from the shard maps
  by ``SLDataset.read_batch`` on a helper thread one batch ahead and uploaded from pinned memory; nothing in the
  loop waits for the GPU -- the epoch's sums are read back once at the end.
* **device-resident fused path** (``SLConfig.device_resident`` or a ``DeviceSLDataset`` handed to the constructor; not in
  the reference): the positions stay packed in device memory, one permutation per epoch is uploaded once, and a
  minibatch is one ``ka_sl_gather`` launch in front of the same per-batch body -- no thread, no pinned copy, no upload
  per batch.  Asked for where the fused path cannot run, it raises instead of falling back.  ``SLConfig.mirror_augment``
  has that gather reflect, left to right, the positions a draw of (``mirror_seed``, epoch, position) names.
  ``SLConfig.visit_targets`` (a dataset with visit rows: the samples of the arena's visit-count search,
  ``SearchSamples.drain()``) has it hand out the visit distribution of every position too, and ``ka_policy_ce_soft`` takes
  the place of ``ka_policy_ce``: the policy loss is the cross-entropy against that distribution.
* **held-out evaluation** (``evaluate()``, not in the reference; the fused path only): eval-mode forwards under ``no_grad``
  over a ``DeviceSLDataset`` -- ``eval_dataset``, typically a tail ``view()`` of the corpus -- one gather and one
  ``ka_sl_eval`` per chunk, the losses as sums over positions and the top-1 / top-k / value hit counts in a 64-byte
  device accumulator that is read once at the end.  Nothing of the training state changes.
* **generic path** (CPU tensors, other models): the reference's loop in ordinary tensor ops.

The shuffling is the reference's: the batch order comes from a ``DataLoader`` (``shuffle=True``) -- over the items on
the generic path, over their indices on the fused path -- so a seeded run visits the positions in the same order.
"""
from __future__ import annotations

import logging
import math
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass, field
from pathlib import Path
from typing import Optional

import torch
import torch.nn.functional as F
from torch.amp import GradScaler, autocast
from torch.utils.data import DataLoader, Dataset, get_worker_info

from keisei_amd import _lib
from keisei_amd.sl.dataset import SLDataset
from keisei_amd.sl.device_dataset import MIRROR_ALL, MIRROR_DRAWN, MIRROR_NONE, DeviceSLDataset
from keisei_amd.training.fused_optim import FusedAdamMixin
from keisei_amd.training.models.katago_base import KataGoBaseModel
from keisei_amd.training.models.se_resnet import SEResNetModel

logger = logging.getLogger(__name__)


@dataclass
class SLConfig:
    data_dir: str
    batch_size: int = 4096
    learning_rate: float = 1e-3
    total_epochs: int = 30
    num_workers: int = 0
    lambda_policy: float = 1.0
    lambda_value: float = 1.5
    lambda_score: float = 0.02
    grad_clip: float = 0.5
    use_amp: bool = False
    allow_placeholder: bool = False
    # the device-resident epoch reflects the drawn positions left to right (keyword-only: device_resident stays the last
    # field and the last positional argument); not in the reference
    mirror_augment: bool = field(default=False, kw_only=True)
    mirror_seed: int = field(default=0, kw_only=True)
    # the policy target is the dataset's visit distribution (a DeviceSLDataset with visit rows, the samples of a visit-count
    # search) and the policy loss ka_policy_ce_soft; keyword-only for the same reason; not in the reference
    visit_targets: bool = field(default=False, kw_only=True)
    device_resident: bool = False          # hold the dataset packed in device memory (DeviceSLDataset); not in the reference

    def __post_init__(self) -> None:
        checks = (("grad_clip", self.grad_clip > 0, "> 0"), ("total_epochs", self.total_epochs >= 0, ">= 0"),
                  ("batch_size", self.batch_size > 0, "> 0"), ("learning_rate", self.learning_rate > 0, "> 0"),
                  ("num_workers", self.num_workers >= 0, ">= 0"))
        for name, ok, bound in checks:
            if not ok:
                raise ValueError(f"{name} must be {bound}, got {getattr(self, name)}")
        # a zero weight switches a head off; a negative one would ascend on it, NaN/inf poison the sum (trainer.py:44-54)
        for name in ("lambda_policy", "lambda_value", "lambda_score"):
            value = getattr(self, name)
            if not math.isfinite(value):
                raise ValueError(f"{name} must be finite, got {value!r}")
            if value < 0:
                raise ValueError(f"{name} must be >= 0, got {value!r}")
        if not -2 ** 63 <= self.mirror_seed < 2 ** 64:
            raise ValueError(f"mirror_seed must fit 64 bits, got {self.mirror_seed!r}")


def _sl_worker_init(worker_id: int) -> None:
    """DataLoader workers reopen the shard maps instead of sharing the parent's (trainer.py:60-71)."""
    info = get_worker_info()
    if info is None:
        return
    ds = info.dataset
    while hasattr(ds, "dataset"):
        ds = ds.dataset
    if hasattr(ds, "clear_cache"):
        ds.clear_cache()


class _Indices(Dataset):
    """0 .. n-1: the sampler machinery of a DataLoader without the per-item decoding."""

    def __init__(self, n: int) -> None:
        self.n = n

    def __len__(self) -> int:
        return self.n

    def __getitem__(self, i: int) -> int:
        return i


class SLTrainer(FusedAdamMixin):
    """Trains one epoch per ``train_epoch()`` call; checkpointing is the caller's business."""

    def __init__(self, model: KataGoBaseModel, config: SLConfig, dataset: Optional[DeviceSLDataset] = None,
                 eval_dataset: Optional[DeviceSLDataset] = None) -> None:
        self.model = model
        self.config = config
        self.device = next(model.parameters()).device
        self.optimizer = torch.optim.Adam(model.parameters(), lr=config.learning_rate)
        on_gpu = self.device.type == "cuda"
        self.scaler = GradScaler(enabled=config.use_amp and on_gpu)
        self.scheduler = torch.optim.lr_scheduler.CosineAnnealingLR(self.optimizer, T_max=max(config.total_epochs, 1),
                                                                    eta_min=1e-6)
        if config.use_amp and (self.device.type == "cpu" or torch.cuda.is_bf16_supported()):
            self._amp_dtype = torch.bfloat16
        else:
            self._amp_dtype = torch.float16          # unused placeholder when AMP is off
        self._amp_device_type = self.device.type
        model.configure_amp(enabled=config.use_amp, dtype=self._amp_dtype, device_type=self._amp_device_type)
        self._hip_state: dict = {}
        self._order_override: Optional[torch.Tensor] = None     # tests: the next device epoch's order instead of randperm
        self.device_dataset: Optional[DeviceSLDataset] = None
        self.eval_dataset = eval_dataset                        # what evaluate() reads when it is given no dataset
        self.epochs_done = 0                                    # train_epoch() calls so far: the epoch of the mirror draw
        if config.mirror_augment and dataset is None and not config.device_resident:
            raise ValueError("mirror_augment reflects positions inside the device-resident gather: it needs "
                             "device_resident=True or a DeviceSLDataset, there is no reflection on the shard path")
        if config.visit_targets and dataset is None and not config.device_resident:
            raise ValueError("visit_targets trains on the visit rows of a device-resident dataset: it needs a "
                             "DeviceSLDataset with visit rows (device_resident=True or dataset=), the shard path has none")
        if dataset is not None or config.device_resident:
            # the positions stay packed on the device and config.data_dir is read at most once, here; there is no other
            # way to run this than the fused path, and no falling back to the shard path
            if not self._fused_path_available():
                raise ValueError("a device-resident dataset needs the fused HIP path: an SEResNetModel on a GPU, fp32 or "
                                 f"bf16 AMP, plain Adam (got {type(model).__name__} on {self.device}, use_amp={config.use_amp})")
            if dataset is None:
                dataset = DeviceSLDataset.from_shards(Path(config.data_dir), device=self.device,
                                                      allow_placeholder=config.allow_placeholder)
            if dataset.device != self.device:
                raise ValueError(f"the dataset lives on {dataset.device}, the model on {self.device}")
            if config.visit_targets and dataset.visits is None:
                raise ValueError("visit_targets=True needs a dataset with visit rows (SearchSamples.drain(), or "
                                 "append_packed(..., visits=)); this dataset holds none")
            self.device_dataset = dataset
            self.dataset = self.dataloader = self._index_loader = None
            return
        self.dataset = SLDataset(Path(config.data_dir), allow_placeholder=config.allow_placeholder)
        has_data = len(self.dataset) > 0
        workers = config.num_workers if has_data else 0
        self.dataloader = DataLoader(self.dataset, batch_size=config.batch_size, shuffle=has_data, num_workers=workers,
                                     pin_memory=on_gpu and workers > 0, persistent_workers=workers > 0,
                                     worker_init_fn=_sl_worker_init if workers > 0 else None)
        self._index_loader = DataLoader(_Indices(len(self.dataset)), batch_size=config.batch_size, shuffle=has_data)

    # ------------------------------------------------------------------ dispatch
    def _fused_path_available(self) -> bool:
        if self.device.type != "cuda" or not isinstance(self.model, SEResNetModel):
            return False
        if self.config.use_amp and self._amp_dtype != torch.bfloat16:
            return False
        return self._fused_optimizer_ok()

    def train_epoch(self) -> dict[str, float]:
        self.model.train()
        if self.device_dataset is not None:
            sums, batches = self._epoch_device()
        elif self._fused_path_available():
            sums, batches = self._epoch_fused()
        else:
            sums, batches = self._epoch_generic()
        self.epochs_done += 1
        if batches > 0:                       # an empty dataset must not burn annealing ticks (trainer.py:176-179)
            self.scheduler.step()
        d = max(batches, 1)
        metrics = {"policy_loss": sums[0] / d, "value_loss": sums[1] / d, "score_loss": sums[2] / d}
        logger.info("SL epoch | policy=%.4f value=%.4f score=%.4f lr=%.6f", metrics["policy_loss"], metrics["value_loss"],
                    metrics["score_loss"], self.optimizer.param_groups[0]["lr"])
        return metrics

    # ------------------------------------------------------------------ generic path (trainer.py:133-174)
    def _epoch_generic(self):
        cfg = self.config
        sums = [0.0, 0.0, 0.0]
        batches = 0
        for batch in self.dataloader:
            obs = batch["observation"].to(self.device)
            tp, tv, ts = (batch[k].to(self.device) for k in ("policy_target", "value_target", "score_target"))
            out = self.model(obs)
            with autocast(device_type=self._amp_device_type, dtype=self._amp_dtype, enabled=cfg.use_amp):
                policy_loss = F.cross_entropy(out.policy_logits.reshape(obs.shape[0], -1), tp)
                value_loss = F.cross_entropy(out.value_logits, tv)
                score_loss = F.mse_loss(out.score_lead.squeeze(-1), ts)
                loss = cfg.lambda_policy * policy_loss + cfg.lambda_value * value_loss + cfg.lambda_score * score_loss
            self.optimizer.zero_grad(set_to_none=True)
            self.scaler.scale(loss).backward()
            self.scaler.unscale_(self.optimizer)
            torch.nn.utils.clip_grad_norm_(self.model.parameters(), cfg.grad_clip)
            self.scaler.step(self.optimizer)
            self.scaler.update()
            eng = getattr(self.model, "_hip_engine", None)
            if eng is not None:
                eng.notify_weights_updated()
            for i, v in enumerate((policy_loss, value_loss, score_loss)):
                sums[i] += v.item()
            batches += 1
        return sums, batches

    # ------------------------------------------------------------------ fused HIP path
    def _fused_begin(self) -> dict:
        """The state of one fused epoch: the Adam tables, the GradScaler's words, the sums and the flags."""
        dev = self.device
        st = self._adam_tables(dev)
        scaler_t = None
        if self.scaler.is_enabled():
            if self.scaler._scale is None:
                self.scaler._lazy_init_scale_growth_tracker(dev)
            scaler_t = torch.stack([self.scaler._scale.float().reshape(()), self.scaler._growth_tracker.float().reshape(())])
        return dict(st=st, sp=_lib.stream_ptr(dev), scaler_t=scaler_t, gscale=scaler_t[0:1] if scaler_t is not None else None,
                    acc=torch.zeros(5, device=dev),            # sums of policy / value / score / (entropy, unused) / grad norm
                    flags=torch.zeros(3, dtype=torch.int32, device=dev),   # non-finite logits, bad policy target, bad gather index
                    out_m=torch.zeros(16, device=dev), A=None)

    def _fused_batch(self, ep: dict, batch: dict) -> None:
        """One minibatch of device tensors: forward, ``ka_policy_ce`` (``ka_policy_ce_soft`` with ``visit_targets``),
        ``ka_value_loss``, backward, ``ka_clip_adam_step``.  The ONE body of the shard epoch and the device-resident epoch."""
        cfg, dev, call = self.config, self.device, _lib.call
        st, sp, scaler_t, gscale, acc, flags = ep["st"], ep["sp"], ep["scaler_t"], ep["gscale"], ep["acc"], ep["flags"]
        group = self.optimizer.param_groups[0]
        beta1, beta2 = group["betas"]
        obs = batch["observation"]
        B = obs.shape[0]
        out = self.model(obs)
        logits = out.policy_logits.reshape(B, -1)
        A = ep["A"] = logits.shape[1]
        dlogits = torch.empty_like(logits)
        rowloss = torch.empty(B, device=dev)
        rowent = torch.zeros(B, device=dev)
        dv, ds = torch.empty(B, 3, device=dev), torch.empty(B, 1, device=dev)
        if cfg.visit_targets:                      # the cross-entropy against the batch's visit distribution
            call("ka_policy_ce_soft", logits, batch["visit_actions"], batch["visit_weights"],
                 int(batch["visit_actions"].shape[1]), dlogits, rowloss, flags, gscale, float(cfg.lambda_policy) / B, B, A, sp)
        else:
            call("ka_policy_ce", logits, batch["policy_target"], None, dlogits, rowloss, flags, gscale,
                 float(cfg.lambda_policy) / B, B, A, sp)
        call("ka_value_loss", out.value_logits, out.score_lead, batch["value_target"], batch["score_target"], None,
             rowloss, rowent, dv, ds, ep["out_m"], acc, gscale, float(cfg.lambda_policy), float(cfg.lambda_value),
             float(cfg.lambda_score), 0.0, 0, B, sp)
        self.optimizer.zero_grad(set_to_none=True)
        torch.autograd.backward([out.policy_logits, out.value_logits, out.score_lead],
                                [dlogits.view_as(out.policy_logits), dv, ds])
        tab = self._upload_table(st, dev)
        call("ka_clip_adam_step", tab, st["blk_t"], st["blk_o"], st["nblocks"], st["partial"], st["ctl"],
             st["step_dev"], scaler_t, flags, acc[4:5], float(cfg.grad_clip), float(group["lr"]), float(beta1),
             float(beta2), float(group["eps"]), sp)
        self.model._hip_engine.notify_weights_updated()
        self.optimizer._opt_called = True          # the scheduler's "step() before optimizer.step()" check

    def _fused_end(self, ep: dict, batches: int):
        if batches == 0:
            return [0.0, 0.0, 0.0], 0
        st, scaler_t = ep["st"], ep["scaler_t"]
        host = torch.cat([ep["acc"], st["step_dev"], ep["flags"].float()]).cpu().tolist()       # the epoch's one read-back
        for q in st["params"]:
            self.optimizer.state[q]["step"].fill_(host[5])
        if scaler_t is not None:
            self.scaler._scale.copy_(scaler_t[0])
            self.scaler._growth_tracker.copy_(scaler_t[1].to(torch.int32))
        if host[8]:
            raise IndexError(f"{int(host[8])} indices outside the dataset reached the gather kernel")
        if host[7]:
            raise ValueError(f"policy_target outside [0, {ep['A']}) reached the loss kernel" if not self.config.visit_targets else
                             f"a visit target outside [0, {ep['A']}), a weight that is negative or not finite, or a position "
                             "without a visited move reached the loss kernel")
        return host[:3], batches

    def _epoch_fused(self):
        dev = self.device
        ep = self._fused_begin()
        batches = 0
        copy_stream = torch.cuda.Stream(dev)
        main = torch.cuda.current_stream(dev)

        def fetch(indices):
            host = self.dataset.read_batch(indices.tolist(), pin=True)
            with torch.cuda.stream(copy_stream):
                devb = {k: v.to(dev, non_blocking=True) for k, v in host.items()}
                ready = torch.cuda.Event()
                ready.record(copy_stream)
            return host, devb, ready

        order = iter(self._index_loader)
        with ThreadPoolExecutor(max_workers=1) as pool:
            first = next(order, None)
            pending = pool.submit(fetch, first) if first is not None else None
            while pending is not None:
                host, batch, ready = pending.result()
                nxt = next(order, None)
                pending = pool.submit(fetch, nxt) if nxt is not None else None
                main.wait_event(ready)
                for t in batch.values():
                    t.record_stream(main)
                self._fused_batch(ep, batch)
                batches += 1
                del host
        return self._fused_end(ep, batches)

    # ------------------------------------------------------------------ device-resident epoch
    def _epoch_device(self):
        """The fused epoch over a ``DeviceSLDataset``: one permutation drawn on the host and uploaded once, then per
        ``batch_size`` slice (the last one partial) one gather launch and the fused batch body."""
        ds, dev = self.device_dataset, self.device
        n = len(ds)
        if n == 0:
            return [0.0, 0.0, 0.0], 0
        order, self._order_override = self._order_override, None
        if order is None:
            order = torch.randperm(n)
        elif order.dtype != torch.int64 or order.dim() != 1:
            raise ValueError("_order_override must be a 1-d int64 tensor")
        order = order.to(dev)
        ep = self._fused_begin()
        gather_flag = ep["flags"][2:3]
        batches = 0
        how = {}
        if self.config.mirror_augment:                           # the draw of (mirror_seed, this epoch, position)
            how = dict(mirror=MIRROR_DRAWN, seed=self.config.mirror_seed, epoch=self.epochs_done)
        if self.config.visit_targets:
            how["visit_targets"] = True
        for lo in range(0, order.shape[0], self.config.batch_size):
            self._fused_batch(ep, ds.gather(order[lo:lo + self.config.batch_size], gather_flag, **how))
            batches += 1
        return self._fused_end(ep, batches)

    # ------------------------------------------------------------------ held-out evaluation
    def evaluate(self, dataset: Optional[DeviceSLDataset] = None, *, batch_size: Optional[int] = None, topk: int = 5,
                 mirror: bool = False) -> dict:
        """Losses and hit rates over ``dataset`` (default ``eval_dataset``) without an update: eval-mode forwards under
        ``no_grad`` in ``batch_size`` chunks (default ``config.batch_size``, the last one partial), each one gather and one
        ``ka_sl_eval``; the accumulator and the flags are read once, at the end.  ``mirror=True`` evaluates the reflected
        positions.  Losses are means over positions (not means of batch means), ``policy_top1`` / ``policy_topk`` the
        fraction of positions whose target move ranks first / among the first ``topk`` logits (ties by the lower index).
        Parameters, BatchNorm buffers, optimiser, scaler, scheduler and every module's train / eval mode are left as found."""
        ds = self.eval_dataset if dataset is None else dataset
        if ds is None:
            raise ValueError("evaluate() needs a dataset: pass one or construct the trainer with eval_dataset=")
        if not self._fused_path_available():
            raise ValueError("evaluate() runs on the fused HIP path only: an SEResNetModel on a GPU, fp32 or bf16 AMP "
                             f"(got {type(self.model).__name__} on {self.device}, use_amp={self.config.use_amp})")
        if ds.device != self.device:
            raise ValueError(f"the dataset lives on {ds.device}, the model on {self.device}")
        chunk = self.config.batch_size if batch_size is None else int(batch_size)
        if chunk < 1:
            raise ValueError(f"batch_size must be > 0, got {batch_size}")
        if topk < 1:
            raise ValueError(f"topk must be >= 1, got {topk}")
        dev, n = self.device, len(ds)
        acc = torch.zeros(8, dtype=torch.int64, device=dev)      # int64[4] counts, then float64[4] sums (ka_sl_eval)
        flags = torch.zeros(3, dtype=torch.int32, device=dev)    # non-finite outputs, bad target, bad gather index
        modes = [(m, m.training) for m in self.model.modules()]
        A = None
        self.model.eval()
        try:
            with torch.no_grad(), torch.cuda.device(dev):
                order = torch.arange(n, device=dev)
                rowloss = torch.empty(min(chunk, n), device=dev)
                rank = torch.empty(min(chunk, n), dtype=torch.int32, device=dev)
                sp = _lib.stream_ptr(dev)
                for lo in range(0, n, chunk):
                    batch = ds.gather(order[lo:lo + chunk], flags[2:3], mirror=MIRROR_ALL if mirror else MIRROR_NONE)
                    B = batch["observation"].shape[0]
                    out = self.model(batch["observation"])
                    logits = out.policy_logits.reshape(B, -1)
                    if A is None:
                        A = logits.shape[1]
                        if topk > A:
                            raise ValueError(f"topk must be <= the {A} actions, got {topk}")
                    if any(t.dtype != torch.float32 for t in (logits, out.value_logits, out.score_lead)):
                        raise _lib.KeiseiHipError("evaluate(): the model's outputs must be fp32")
                    _lib.call("ka_sl_eval", logits.contiguous(), out.value_logits.contiguous(),
                              out.score_lead.reshape(B).contiguous(), batch["policy_target"], batch["value_target"],
                              batch["score_target"], B, A, int(topk), rowloss, rank, acc, flags, sp)
        finally:
            for m, was in modes:
                m.training = was
        host = torch.cat([acc, flags.to(torch.int64)]).cpu()     # the one read-back
        counts, sums = host[:4].tolist(), host[4:8].view(torch.float64).tolist()
        nan, bad_target, bad_index = host[8:].tolist()
        if bad_index:
            raise IndexError(f"{bad_index} indices outside the dataset reached the gather kernel")
        if nan:
            raise ValueError("non-finite model outputs reached the evaluation kernel")
        if bad_target:
            raise ValueError(f"a policy target outside [0, {A}) or a value target outside {{0, 1, 2}} reached the "
                             "evaluation kernel")
        d = max(counts[0], 1)
        return {"policy_loss": sums[0] / d, "value_loss": sums[1] / d, "score_loss": sums[2] / d,
                "policy_top1": counts[1] / d, "policy_topk": counts[2] / d, "value_accuracy": counts[3] / d,
                "positions": int(counts[0])}
