"""Grouped eval forward: many SE-ResNets of one shape over one board batch.

League and tournament play evaluate many resident models at once, each on a handful of boards (the reference's
``ConcurrentMatchPool.run_round`` Phase 2, concurrent_matches.py:353-364, and the cohort loop of ``split_merge_step``,
katago_loop.py:404-431: one forward per model).  ``SEResNetGroup`` runs them as ONE forward: board b is evaluated by
``models[model_idx[b]]``, and on a GPU the whole batch is three kernel launches (grouped stem, grouped residual tower,
grouped heads: csrc/tower.hip) whatever the number of models, with no host synchronisation when ``check=False`` -- so a
caller may capture it in a graph.

Eval mode, no autograd, bf16 activations on the GPU (the reference's production arithmetic).  CPU models take a plain
loop over the models' own ``nn`` forwards (in eval mode) on their rows.
"""
from __future__ import annotations

from typing import Optional, Sequence, Tuple

import torch

from .models.katago_base import KataGoOutput
from .models.se_resnet import SEResNetModel

_ACTIONS = 81 * SEResNetModel.SPATIAL_MOVE_TYPES


class SEResNetGroup:
    """K ``SEResNetModel`` instances with identical ``SEResNetParams`` on one device, evaluated together.

    ``forward`` sees the models as of the last ``refresh()`` on a GPU: the group holds its own snapshot of packed weights,
    BatchNorm eval coefficients and FC weights.  Call ``refresh()`` after an optimiser step, a ``load_state_dict`` or any
    other in-place edit of weights or running statistics.  (On the CPU the loop calls the models themselves and always sees
    their current state.)  Replacing a parameter tensor (``model.to(...)``, assigning a new ``nn.Parameter``) is not an
    in-place edit: build a new group."""

    def __init__(self, models: Sequence[SEResNetModel], *, dtype: torch.dtype = torch.bfloat16) -> None:
        models = list(models)
        if not models:
            raise ValueError("SEResNetGroup needs at least one model")
        for i, m in enumerate(models):
            if not isinstance(m, SEResNetModel):
                raise ValueError(f"model {i} is a {type(m).__name__}, not an SEResNetModel")
        p0 = models[0].params
        for i, m in enumerate(models[1:], 1):
            if m.params != p0:
                raise ValueError(f"models differ in SEResNetParams: model 0 has {p0}, model {i} has {m.params}")
        devs = {t.device for m in models for t in (*m.parameters(), *m.buffers())}
        if len(devs) != 1:
            raise ValueError(f"models sit on different devices: {sorted(str(d) for d in devs)}")
        self.models = models
        self.params = p0
        self.device = devs.pop()
        self.dtype = dtype
        self._tables = None
        if self.device.type == "cuda":
            self._validate_gpu()
            from keisei_amd.hip.group import GroupTables
            with torch.cuda.device(self.device):
                self._tables = GroupTables(models, self.device)
        self.refresh()

    def __len__(self) -> int:
        return len(self.models)

    def _validate_gpu(self) -> None:
        from keisei_amd import _lib

        p = self.params
        if self.dtype != torch.bfloat16:
            raise ValueError(f"the grouped GPU forward runs bf16 activations only (dtype={self.dtype})")
        m0 = self.models[0]
        G, R = m0.blocks[0].global_fc[0].out_features, m0.blocks[0].se_fc1.out_features
        if not _lib.query("ka_tower_eval_grouped_supported", p.channels, G, R, _lib.DTYPE_BF16):
            raise ValueError(f"the grouped kernels do not cover this shape: channels={p.channels} (128 or 256), "
                             f"global_pool_channels={G} (8..256, a multiple of 8), channels // se_reduction={R} (1..64)")
        if p.policy_channels > 32 or p.value_fc_size > 512 or p.score_fc_size > 512 or p.obs_channels > 128:
            raise ValueError(f"the grouped heads do not cover this shape: policy_channels={p.policy_channels} (<= 32), "
                             f"value_fc_size={p.value_fc_size}, score_fc_size={p.score_fc_size} (<= 512), "
                             f"obs_channels={p.obs_channels} (<= 128)")
        for i, m in enumerate(self.models):
            for name, t in (*m.named_parameters(), *m.named_buffers()):
                if t.is_floating_point() and t.dtype != torch.float32:
                    raise ValueError(f"model {i}: {name} is {t.dtype} (the grouped kernels read fp32 parameters)")
            for name, t in m.named_buffers():
                if name.endswith(("running_mean", "running_var")) and t is None:
                    raise ValueError(f"model {i}: BatchNorm without running statistics ({name})")

    def refresh(self) -> None:
        """Re-derive the group's packs, BatchNorm coefficients and FC copies from the models' current state."""
        if self._tables is not None:
            with torch.cuda.device(self.device), torch.no_grad():
                self._tables.refresh()

    # ------------------------------------------------------------------ forward
    def _model_idx(self, model_idx: torch.Tensor, B: int, check: bool) -> torch.Tensor:
        if model_idx.ndim != 1 or model_idx.shape[0] != B:
            raise ValueError(f"model_idx must have shape ({B},), got {tuple(model_idx.shape)}")
        if model_idx.dtype.is_floating_point or model_idx.dtype == torch.bool:
            raise ValueError(f"model_idx must be an integer tensor, got {model_idx.dtype}")
        if check and B > 0:
            lo, hi = torch.aminmax(model_idx)
            lo, hi = torch.stack((lo, hi)).tolist()           # the one device -> host read of a checked forward
            if hi >= len(self.models) or lo < -1:
                raise ValueError(f"model_idx out of range: values in [{lo}, {hi}], the group holds {len(self.models)} "
                                 "models (-1 = unseated)")
        return model_idx

    def forward(self, obs: torch.Tensor, model_idx: torch.Tensor, *, check: bool = True) -> KataGoOutput:
        """Board b of ``obs`` (B, 50, 9, 9) evaluated by ``models[model_idx[b]]``; ``model_idx = -1`` (unseated) gives zero
        outputs.  ``check=True`` rejects indices outside [-1, K) with one device -> host read; with ``check=False`` the
        kernels treat any index outside [0, K) as unseated."""
        self.models[0]._check_obs(obs)
        B = obs.shape[0]
        model_idx = self._model_idx(model_idx, B, check)
        with torch.no_grad():
            if self._tables is None:
                return self._forward_cpu(obs, model_idx)
            dev = self.device
            if obs.device != dev:
                raise ValueError(f"obs is on {obs.device}, the group on {dev}")
            obs = obs if (obs.dtype == torch.float32 and obs.is_contiguous()) else obs.float().contiguous()
            mo = model_idx.to(device=dev, dtype=torch.int32).contiguous()
            if B == 0:
                z = obs.new_zeros
                return KataGoOutput(z(0, 9, 9, SEResNetModel.SPATIAL_MOVE_TYPES), z(0, 3), z(0, 1))
            with torch.cuda.device(dev):
                logits, value, score = self._tables.forward(obs, mo)
            return KataGoOutput(policy_logits=logits, value_logits=value, score_lead=score)

    __call__ = forward

    def _forward_cpu(self, obs: torch.Tensor, model_idx: torch.Tensor) -> KataGoOutput:
        B = obs.shape[0]
        idx = model_idx.to(obs.device)
        policy = obs.new_zeros(B, 9, 9, SEResNetModel.SPATIAL_MOVE_TYPES, dtype=torch.float32)
        value = obs.new_zeros(B, 3, dtype=torch.float32)
        score = obs.new_zeros(B, 1, dtype=torch.float32)
        for k, m in enumerate(self.models):
            rows = (idx == k).nonzero(as_tuple=True)[0]
            if rows.numel() == 0:
                continue
            was = m.training
            m.eval()
            try:
                o = m(obs[rows])
            finally:
                m.train(was)
            policy[rows] = o.policy_logits.float()
            value[rows] = o.value_logits.float()
            score[rows] = o.score_lead.float()
        return KataGoOutput(policy_logits=policy, value_logits=value, score_lead=score)

    # ------------------------------------------------------------------ sampling
    def select_actions(self, obs: torch.Tensor, legal_masks: torch.Tensor, model_idx: torch.Tensor,
                       seed: Optional[int] = None, *, check: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
        """(actions (B,) int64, log_probs (B,) fp32) sampled from each board's own model.  ``legal_masks``: bool
        (B, 11259) / (B, 9, 9, 139), or packed int32 rows (B, 352) as ``ka_policy_sample`` accepts.  Unseated rows get
        action -1 and log-prob 0.  Without a seed one is drawn from torch's host generator, as select_actions does."""
        B = obs.shape[0]
        out = self.forward(obs, model_idx, check=check)
        if seed is None:
            seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        words = (_ACTIONS + 31) // 32
        if legal_masks.dtype == torch.bool:
            masks = legal_masks.reshape(B, _ACTIONS)
            legal_words = 0
        elif legal_masks.dtype == torch.int32 and legal_masks.shape == (B, words):
            masks, legal_words = legal_masks, words
        else:
            raise ValueError(f"legal_masks must be bool (B, {_ACTIONS}) or packed int32 (B, {words}), "
                             f"got {legal_masks.dtype} {tuple(legal_masks.shape)}")
        seated = (model_idx >= 0) & (model_idx < len(self.models))
        if self._tables is None:
            return self._sample_cpu(out.policy_logits.reshape(B, _ACTIONS), masks, legal_words, seated.to(obs.device), seed)
        from keisei_amd import _lib

        dev = self.device
        logits = out.policy_logits.reshape(B, _ACTIONS)
        masks = masks.to(dev).contiguous()
        actions = torch.empty(B, dtype=torch.int64, device=dev)
        log_probs = torch.empty(B, device=dev)
        n_legal = torch.empty(B, dtype=torch.int32, device=dev)
        flags = torch.zeros(2, dtype=torch.int32, device=dev)
        if B == 0:
            return actions, log_probs
        with torch.cuda.device(dev):
            _lib.call("ka_policy_sample", logits, 0, masks, legal_words, seed, None, None, 0.0, actions, log_probs, None,
                      n_legal, flags, B, _ACTIONS, _lib.stream_ptr(dev))
        nan_seen, zero_legal = flags.tolist()
        seated = seated.to(dev)
        if zero_legal:
            empty = ((n_legal == 0) & seated).nonzero(as_tuple=True)[0].tolist()
            if empty:                                       # katago_ppo.py:589-596
                raise RuntimeError(f"Environments {empty} have zero legal actions — "
                                   f"all-False legal mask would produce NaN")
        if nan_seen:
            raise RuntimeError("NaN in raw policy logits in select_actions — probability tensor contains nan "
                               "(the model has diverged)")
        actions = torch.where(seated, actions, torch.full_like(actions, -1))
        log_probs = torch.where(seated, log_probs, torch.zeros_like(log_probs))
        return actions, log_probs

    def _sample_cpu(self, logits, masks, legal_words, seated, seed):
        B = logits.shape[0]
        if legal_words:
            bits = torch.arange(_ACTIONS)
            masks = ((masks[:, bits // 32] >> (bits % 32)) & 1).bool()
        if torch.isnan(logits).any():
            raise RuntimeError("NaN in raw policy logits in select_actions — probability tensor contains nan "
                               "(the model has diverged)")
        n_legal = masks.sum(dim=-1)
        empty = ((n_legal == 0) & seated).nonzero(as_tuple=True)[0].tolist()
        if empty:
            raise RuntimeError(f"Environments {empty} have zero legal actions — all-False legal mask would produce NaN")
        actions = torch.full((B,), -1, dtype=torch.int64)
        log_probs = torch.zeros(B)
        rows = seated.nonzero(as_tuple=True)[0]
        if rows.numel():
            g = torch.Generator().manual_seed(seed & (2 ** 63 - 1))
            lp = torch.log_softmax(logits[rows].float().masked_fill(~masks[rows], float("-inf")), dim=-1)
            a = torch.multinomial(lp.exp(), 1, generator=g).squeeze(1)
            actions[rows] = a
            log_probs[rows] = lp.gather(1, a.unsqueeze(1)).squeeze(1)
        return actions, log_probs
