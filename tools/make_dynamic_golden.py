"""Generates tests/golden/g11_dynamic.npz: the reference's DynamicTrainer.update() on a 2 x 32 se_resnet (dev container only:
imports the reference tree named by KEISEI_REFERENCE; copies none of its code).

The reference's class runs unchanged on a stub store, twice: in fp64 (model and inputs cast to double) and in fp32 under
several permutation seeds.  The fixture holds the inputs (four small rollouts, two per side, masks packed), the initial
state_dict, the fp64 state_dict after update(), the fp64 old_log_probs (in batch order), Adam's exp_avg of the first
parameter, and per tensor d_ref = the largest distance of any fp32 run from the fp64 run.

learner_lr = 1e-3 with the default DynamicConfig (lr = 2.5e-4, two epochs).  The test's floor per tensor is
0.05 x epochs x lr = 2.5e-5: if the repeats printed below come within a factor three of it, change the inputs, not the bar.

    python tools/make_dynamic_golden.py [--out tests/golden/g11_dynamic.npz]
"""
from __future__ import annotations

import argparse
import copy
import importlib
import os
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
REF = Path(os.environ.get("KEISEI_REFERENCE", "/root/reference"))
sys.path.insert(0, str(ROOT))
sys.dont_write_bytecode = True

from oracle import keisei_oracle as orc  # noqa: E402

SHAPE = orc.NetShape(2, 32, 8, 16, 8, 32, 16)
A, WORDS = 11259, 352
STEPS, ENVS = 6, 2
SEEDS = (0, 1, 2, 3, 4, 5)
LEARNER_LR = 1e-3


def _rollout_arrays(k: int) -> dict:
    """rollout k: (STEPS, ENVS) rows, movers alternating, terminal rows with a win, a loss and a draw for both sides"""
    g = torch.Generator().manual_seed(100 + k)
    obs = (torch.rand(STEPS, ENVS, 50, 9, 9, generator=g) < 0.12).float()
    masks = torch.rand(STEPS, ENVS, A, generator=g) < 0.004
    actions = torch.randint(0, A, (STEPS, ENVS), generator=g)
    masks.scatter_(2, actions.unsqueeze(-1), True)
    persp = (torch.arange(STEPS)[:, None] + torch.arange(ENVS)[None, :] + k) % 2
    rewards, dones = torch.zeros(STEPS, ENVS), torch.zeros(STEPS, ENVS)
    # (step, env, reward): both parities of step + env + k are hit with +1, -1 and 0
    for t, e, r in ((1, 0, 1.0), (2, 0, -1.0), (3, 0, 0.0), (2, 1, 1.0), (3, 1, -1.0), (4, 1, 0.0)):
        rewards[t, e], dones[t, e] = r, 1.0
    return {"observations": obs, "actions": actions, "rewards": rewards, "dones": dones, "legal_masks": masks,
            "perspective": persp.to(torch.long)}


def _pack(masks: torch.Tensor) -> np.ndarray:
    flat = masks.reshape(-1, A).numpy()
    padded = np.zeros((flat.shape[0], WORDS * 32), dtype=np.uint8)
    padded[:, :A] = flat
    return np.packbits(padded.reshape(-1, WORDS, 32), axis=-1, bitorder="little").view("<u4").reshape(-1, WORDS).view(np.int32)


class _Entry:
    id = 7


class _Store:
    def __init__(self, model):
        self.model, self.saved, self.opt = model, None, None

    def load_opponent(self, entry, device):
        return copy.deepcopy(self.model).to(device).eval()

    def load_optimizer(self, entry_id):
        return None

    def save_weights(self, entry_id, sd):
        self.saved = {k: v.detach().clone() for k, v in sd.items()}

    def save_optimizer(self, entry_id, sd):
        self.opt = sd

    def increment_update_count(self, entry_id):
        pass

    def get_entry(self, entry_id):
        return None


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=str(ROOT / "tests" / "golden" / "g11_dynamic.npz"))
    args = ap.parse_args()
    if not (REF / "keisei").is_dir():
        sys.exit(f"needs the reference tree at {REF} (dev container only)")
    sys.path.insert(0, str(REF))
    try:
        import tomllib  # noqa: F401
    except ModuleNotFoundError:
        sys.modules["tomllib"] = importlib.import_module("tomli")
    import enum
    if not hasattr(enum, "StrEnum"):
        class StrEnum(str, enum.Enum):
            def __str__(self) -> str:
                return str(self.value)

        enum.StrEnum = StrEnum
    ref_dt = importlib.import_module("keisei.training.dynamic_trainer")
    ref_cfg = importlib.import_module("keisei.config")
    ref_reg = importlib.import_module("keisei.training.model_registry")

    sd0 = orc.init_like_state_dict(SHAPE, salt=7)
    model = ref_reg.build_model("se_resnet", dict(SHAPE.__dict__))
    model.load_state_dict(sd0, strict=True)
    rollouts = [_rollout_arrays(k) for k in range(4)]
    sides = [0, 0, 1, 1]

    def run(dtype, seed):
        store = _Store(copy.deepcopy(model).to(dtype))
        tr = ref_dt.DynamicTrainer(store, ref_cfg.DynamicConfig(), LEARNER_LR)
        for r, side in zip(rollouts, sides):
            cast = {k: (v.to(dtype) if v.dtype == torch.float32 else v) for k, v in r.items()}
            tr.record_match(_Entry.id, ref_dt.MatchRollout(**cast), side)
        seen = {}
        real_loss, real_perm = ref_dt.ppo_clip_loss, torch.randperm

        def spy_perm(n, *a, **k):
            p = real_perm(n, *a, **k)
            seen.setdefault("perm", p.clone())
            return p

        def spy_loss(new_lp, old_lp, adv, **k):
            if "old" not in seen:
                old = torch.empty_like(old_lp)
                old[seen["perm"]] = old_lp.detach()
                seen["old"] = old
            return real_loss(new_lp, old_lp, adv, **k)

        torch.manual_seed(seed)
        ref_dt.ppo_clip_loss, torch.randperm = spy_loss, spy_perm
        try:
            assert tr.update(_Entry(), "cpu") is True
        finally:
            ref_dt.ppo_clip_loss, torch.randperm = real_loss, real_perm
        opt = tr._optimizers[_Entry.id]
        first = opt.param_groups[0]["params"][0]
        return store.saved, seen["old"], opt.state[first]["exp_avg"].clone()

    sd64, old64, m64 = run(torch.float64, 0)
    runs32 = [run(torch.float32, s) for s in SEEDS]
    d_ref, spread, beyond = {}, 0.0, 0
    for k, v in sd64.items():
        if not v.dtype.is_floating_point:
            continue
        d_ref[k] = max(float((r[0][k].double() - v).abs().max()) for r in runs32)
        for r in runs32[1:]:
            diff = (r[0][k] - runs32[0][0][k]).abs()
            spread = max(spread, float(diff.max()))
            beyond += int((diff > 3e-5).sum())
    floor = 0.05 * ref_cfg.DynamicConfig().update_epochs_per_batch * LEARNER_LR * ref_cfg.DynamicConfig().lr_scale
    worst = max(d_ref, key=d_ref.get)
    print(f"fp32 against fp64: worst tensor {worst} {d_ref[worst]:.3e}; fp32 runs among themselves: {spread:.3e}, "
          f"{beyond} elements beyond 3e-5; floor {floor:.3e}")
    assert max(d_ref[worst], spread) * 3 < floor, "the repeats come within a factor three of the floor: change the inputs"

    out = {}
    for i, (r, side) in enumerate(zip(rollouts, sides)):
        out[f"r{i}.observations"] = r["observations"].numpy().astype(np.uint8)          # 0 / 1 planes
        out[f"r{i}.legal_mask_bits"] = _pack(r["legal_masks"]).reshape(STEPS, ENVS, WORDS)
        for k in ("actions", "rewards", "dones", "perspective"):
            out[f"r{i}.{k}"] = r[k].numpy()
        out[f"r{i}.side"] = np.int64(side)
    for k, v in sd0.items():
        out["sd0." + k] = v.numpy()
    for k, v in sd64.items():
        out["sd1." + k] = v.numpy()
        if k in d_ref:
            out["dref." + k] = np.float64(d_ref[k])
    out["old_log_probs"] = old64.numpy()
    out["opt.exp_avg.0"] = m64.numpy()
    out["learner_lr"] = np.float64(LEARNER_LR)
    np.savez_compressed(args.out, **out)
    print(f"wrote {args.out} ({Path(args.out).stat().st_size} bytes)")


if __name__ == "__main__":
    main()
