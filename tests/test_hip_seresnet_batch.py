"""GPU: the SE-ResNet HIP engine at training batch sizes against the functional oracle (oracle.keisei_oracle.seresnet_forward,
pinned by test_oracle_golden.py and test_seresnet_oracle_cpu.py) run in float64 with autograd on the device.

The engine changes kernels with the batch size: from 512 boards on the bf16 mode leaves conv3x3_kernel for the two-board
kernel (conv3x3_pc2_kernel), computes square 80 of the 256-channel tower inside it or in conv3x3_corner_kernel (32 boards
per workgroup), and no longer forms dz (ka_block_dx_tail_bwd_du_gate + ka_conv3x3_dgrad_fused_gated); the weight gradient's
split count, the BatchNorm partial rows, the FC split-K and the side-stream fork (B < 512) depend on B as well.  Towers:
c256 = 2x256 (five-row tiles, pc2, corner, gate form), c128 = 3x128 (pc2 without the corner, gate form), c96 = 2x96 with small
heads (generic route at every B, no gate form).  Batches: 1, 2, 65, 511 / 512 (both sides of every B switch), 515 (odd: a
half-empty last pair, 3 boards in the last corner group), 1031 (prime), 4096 (the bench batch; c256 and c128).

fp32 mode is held to rtol 1e-4 / atol 5e-5 on the outputs and 5e-5 on every gradient tensor (norm and relative L2), train
and eval.  At these sizes a handful of ReLU inputs and, now and then, one global-pool maximum lie within fp32 rounding of a
tie, and two correct fp32 implementations that take different sides are 1e-3 apart in gradients.  So the fp64 reference
takes the HIP run's decisions -- the ones its BACKWARD gates on: `> 0` on the stored post-ReLU tensors, the recomputed
fma(y, scale, shift) > 0 where the backward recomputes (stem, bn1, policy_bn1: one v_pk_fma_f32 / v_fmac_f32 in the ISA of
relu_bn_bwd_reduce_kernel / rows_bn_bwd_kernel), x == max on the saved block input and pool row -- after checking that every
decision that differs from the plain fp64 run is a tie (TIE, TIE_FRACTION below).

bf16 mode: the forward against the oracle's bf16-storage emulation (the engine must be nearer to it than it is to fp64),
the gradients against fp64 with the oracle's own bf16 autocast run on the device as the yardstick, measured live; the launch
counters (ka_conv_route_counts) and the engine's `supported` queries show which kernels ran; then each KA_* route switch
against the default.

Measured on MI355X: the 86 cases of this file take 11 s in one process (the fp64 oracle takes its convolutions as one GEMM
over gathered taps); peak device memory 49.7 GiB, in the 4096-board case of c256.  The per-case figures are in the table
above _fp32_train."""
from functools import lru_cache

import pytest
import torch

from keisei_amd import _lib
from keisei_amd.hip.seresnet import SEResNetEngine
from keisei_amd.training.models.se_resnet import SEResNetModel, SEResNetParams
from oracle import keisei_oracle as orc

pytestmark = pytest.mark.gpu
DEV = "cuda"

TOWERS = {"c256": orc.NetShape(2, 256), "c128": orc.NetShape(3, 128), "c96": orc.NetShape(2, 96, 8, 24, 8, 40, 24)}
BATCHES = (1, 2, 65, 511, 512, 515, 1031)
CASES = [(t, B) for t in TOWERS for B in BATCHES + ((4096,) if t != "c96" else ())]

# ---- fp32 mode.  Bounds from the project, none measured on this engine: the outputs at test_hip_model.py's rtol / atol, every
# gradient tensor at its MID_GRAD_TOL (set there for tie-free batches, which is what following the decisions produces; the torch
# fp32 run of the oracle itself lands at 3.3e-6 or better from the followed fp64 run on these cases).
OUT_RTOL, OUT_ATOL = 1e-4, 5e-5
FP32_TOL = 5e-5
# A followed decision must be a tie: a ReLU decision may differ from the sign of the fp64 input only where |input| <= TIE x the
# largest |input| of its layer, an amax winner set from fp64's only where the gap to the fp64 maximum is <= TIE x the largest
# |value| of that pool input, and at most TIE_FRACTION of a case's decisions may differ.  (torch fp32 against fp64 on these
# cases: 1.3e-7, 1.2e-7, 2.8e-7 -- the caps leave a factor 35 to 80 for another summation order; a mask taken from the wrong
# board or layer differs in far more than one decision in 1e5.)
TIE, TIE_FRACTION = 1e-5, 1e-5

# ---- bf16 mode.  Forward: ||hip - emulation|| <= EMU_FACTOR x ||emulation - fp64|| on the policy logits (an emulation that
# rounds where the engine stores bf16 is by construction the nearer neighbour).  Gradients, per-tensor relative L2 from fp64:
# median <= MED_FACTOR x and worst <= WORST_FACTOR x the same figures of the oracle under torch.autocast(bfloat16) on the device
# (test_hip_model.py's record at 16 boards: engine / reference 0.86-0.96 median, 0.69-1.25 worst; the worst rounded up a step).
EMU_FACTOR, MED_FACTOR, WORST_FACTOR = 1.0, 1.25, 1.5

ROUTES = ("conv", "pc", "pc2", "pc2_corner_in", "pc2_corner_out", "corner", "wgrad_lean", "wgrad_tiled")


def _routes():
    out = torch.zeros(len(ROUTES), dtype=torch.int64)
    _lib.call("ka_conv_route_counts", out.data_ptr(), len(ROUTES))
    return out


# ------------------------------------------------------------------ one (tower, batch): model, inputs, fp64 references
class _Case:
    pass


def _model(tower, momentum=0.0):
    shape = TOWERS[tower]
    m = SEResNetModel(SEResNetParams(**shape.__dict__))
    m.load_state_dict(orc.init_like_state_dict(shape), strict=True)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.momentum = momentum
    return m.to(DEV)


def _oracle(c, dt, train, grad, autocast=False, **kw):
    """Oracle outputs (and parameter gradients of (p * cp).sum() / B + (v * cv).sum() + (s * cs).sum()) in dt on the device.
    (cudnn.flags: BatchNorm on torch's own kernels -- the vendor library compiles its kernels per shape on first use.)"""
    sd = {k: (v.to(DEV, dt) if v.dtype.is_floating_point else v.to(DEV)) for k, v in c.sd.items()}
    leaves = {k: v.requires_grad_(True) for k, v in sd.items() if v.dtype.is_floating_point and "running" not in k} if grad else {}
    with torch.set_grad_enabled(grad), torch.backends.cudnn.flags(enabled=False):
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            p, v, s = orc.seresnet_forward(sd, c.obs.to(dt), c.nb, train, momentum=0.0, **kw)
        outs = (p.detach().to(dt), v.detach().to(dt), s.detach().to(dt))
        if not grad:
            return outs, None
        loss = (p.to(dt) * c.cp.to(dt)).sum() / c.B + (v.to(dt) * c.cv.to(dt)).sum() + (s.to(dt) * c.cs.to(dt)).sum()
        grads = dict(zip(leaves, torch.autograd.grad(loss, list(leaves.values()))))
    return outs, grads


@lru_cache(maxsize=1)
def _case(tower, B):
    torch.cuda.empty_cache()
    c = _Case()
    c.tower, c.B, c.nb, c.C = tower, B, TOWERS[tower].num_blocks, TOWERS[tower].channels
    c.sd = orc.init_like_state_dict(TOWERS[tower])
    c.m = _model(tower)
    c.obs = orc.board_like_obs(B, seed=B).to(DEV)
    c.cp, c.cv, c.cs = (t.to(DEV) for t in orc.closed_form_cotangents(B))
    c.relu_taps, c.pool_taps = [], []
    c.ref_train, c.ref_grads = _oracle(c, torch.float64, True, True, relu_inputs=c.relu_taps, pool_inputs=c.pool_taps)
    c.ref_eval, _ = _oracle(c, torch.float64, False, False)
    c.lazy = {}
    return c


def _emulation(c, train):
    key = ("emu", train)
    if key not in c.lazy:
        c.lazy[key] = _oracle(c, torch.float64, train, False, bf16_storage=True)[0]
    return c.lazy[key]


def _yardstick(c):
    """(median, worst) per-tensor relative L2 from fp64 of the oracle's gradients under torch.autocast(bfloat16) on the device"""
    if "yard" not in c.lazy:
        _, g = _oracle(c, torch.float32, True, True, autocast=True)
        l2 = sorted(e[1] for e in _grad_errs(g, c.ref_grads).values())
        c.lazy["yard"] = (l2[len(l2) // 2], l2[-1])
    return c.lazy["yard"]


def _engine(c, T, train, backward=True, obs=None, idx=None):
    """One forward (+ backward) of a fresh engine: outputs, gradients, the saved tensors, the launch counts."""
    eng = SEResNetEngine(c.m)
    before = _routes()
    with torch.no_grad():
        pol, val, sco, sv = eng.forward(c.obs if obs is None else obs, train, True, T, idx)
        grads = eng.backward(sv, c.cp / c.B, c.cv, c.cs) if backward else None
    torch.cuda.synchronize()
    return (pol.float(), val.float(), sco.float()), grads, sv, dict(zip(ROUTES, (_routes() - before).tolist()))


# ------------------------------------------------------------------ comparisons
def _close(got, ref):
    """max |got - ref| / (atol + rtol |ref|): <= 1 is torch.allclose"""
    return float(((got.double() - ref.double()).abs() / (OUT_ATOL + OUT_RTOL * ref.double().abs())).max())


def _grad_errs(grads, ref):
    """per tensor (|norm / reference norm - 1|, relative L2 against the reference)"""
    out = {}
    for n, r in ref.items():
        g, rn = grads[n].double().reshape(r.shape), float(r.norm())
        assert bool(torch.isfinite(g).all()), n
        if rn == 0:
            assert float(g.norm()) == 0, n
            continue
        out[n] = (abs(float(g.norm()) - rn) / rn, float((g - r).norm()) / rn)
    return out


def _nchw(t, B):
    """(B, 81, C) or (B * 81, C) activation of the engine -> (B, C, 9, 9)"""
    return t.reshape(B, 81, -1).permute(0, 2, 1).reshape(B, -1, 9, 9)


def _bn_relu_decision(y, sc, sh):
    """What the backward kernels recompute, fma(y, scale, shift) > 0 (a fused multiply-add of three floats is the float of the
    exact sum in float64), and how many elements decide otherwise as a multiply and an add."""
    y = y.float().reshape(-1, sc.numel())
    fused = (y.double() * sc.double() + sh.double()).float() > 0
    unfused = (y * sc + sh) > 0
    return fused, fused != unfused


def _decisions(c, sv):
    """ReLU masks in the oracle's call order, amax winner sets per global_pool call, from the saved tensors of an fp32 run;
    and the elements whose sign depends on whether y * scale + shift is fused, for the stem and the policy head."""
    B = c.B
    relu, winners, order = [], [], {}
    y0, sc0, sh0 = sv.stem[:3]
    m0, order["stem"] = _bn_relu_decision(y0, sc0, sh0)
    relu.append(_nchw(m0, B))
    for (bx, bpool, y1, sc1, sh1, mu1, is1, g1, g, y2, sc2, sh2, mu2, is2, sqz, se1, se, out, x2) in sv.blocks:
        m1, order[f"bn1[{len(winners)}]"] = _bn_relu_decision(y1, sc1, sh1)
        relu += [_nchw(m1, B), g1 > 0, se1 > 0, _nchw(out > 0, B)]
        winners.append((bx, bpool))
    x, pool, p1, scp, shp, mup, isp, p1r, v1, s1 = sv.heads
    mp, order["policy"] = _bn_relu_decision(p1, scp, shp)
    relu += [_nchw(mp, B), v1 > 0, s1 > 0]
    winners.append((x, pool))
    sets = []
    for xx, pl in winners:
        C = xx.shape[2]
        w = xx == pl[:, None, C:2 * C]                      # the comparison of block_dx_kernel: saved input against saved max
        assert torch.equal(w.sum(dim=1).float(), pl[:, 3 * C:]), "the pool row's tie count is not the number of squares at the maximum"
        sets.append(w.permute(0, 2, 1))
    # the forward's stored post-ReLU tensor against the backward's recomputation: they may differ only where the order of the
    # multiply-add decides
    fwd_stem = (sv.blocks[0][0] if sv.blocks else x).reshape(m0.shape) > 0
    for name, fwd, bwd in (("stem", fwd_stem, m0), ("policy", p1r > 0, mp)):
        bad = int(((fwd != bwd) & ~order[name]).sum())
        assert bad == 0, f"{name}: the forward's ReLU and the backward's recomputed mask disagree on {bad} elements"
    return relu, sets, {k: int(v.sum()) for k, v in order.items()}


def _check_ties(c, relu, sets):
    """Every decision of the HIP run that differs from the plain fp64 run must be a tie; returns the counts."""
    n_relu = n_pool = total = 0
    for k, (a, r) in enumerate(zip(c.relu_taps, relu)):
        differ = (a > 0) != r.reshape(a.shape)
        total += a.numel()
        n = int(differ.sum())
        if n:
            worst, scale = float(a[differ].abs().max()), float(a.abs().max())
            assert worst <= TIE * scale, (f"ReLU {k}", n, worst, scale)
            n_relu += n
    for k, (f, w) in enumerate(zip(c.pool_taps, sets)):
        mx = f.amax(dim=2, keepdim=True)
        differ = w != (f == mx)
        total += f.shape[0] * f.shape[1]
        n = int(differ.any(dim=2).sum())
        if n:
            gap, scale = float((mx - f)[differ].max()), float(f.abs().max())
            assert gap <= TIE * scale, (f"pool {k}", n, gap, scale)
            n_pool += n
    assert len(relu) == len(c.relu_taps) and len(sets) == len(c.pool_taps)
    assert n_relu + n_pool <= TIE_FRACTION * total, (n_relu, n_pool, total)
    return n_relu, n_pool, total


# ---- measured on MI355X (nothing below is a bound).  fp32 train: worst / median relative L2 over the gradient tensors against the
# followed fp64 run, the outputs as a fraction of the tolerance, decisions followed (ReLU + amax winner sets, of how many
# decisions).  bf16: ||hip - emulation|| / ||emulation - fp64|| on the policy logits, train / eval; gradient relative L2 from
# fp64, median / worst, the oracle's under autocast in brackets, and the two quotients the margins apply to.
#   tower      B | fp32 worst / median       outputs  followed                    | bf16 emulation   gradients median / worst (oracle autocast)  quotients
#   c256      1 | 2.79e-06 / 1.54e-06   0.042     0 + 0 of    0.11 M | 0.380 / 0.000;  0.1038 / 0.2100 (0.1096 / 0.2324)  0.947 / 0.904
#   c256      2 | 2.90e-06 / 1.56e-06   0.060     0 + 0 of    0.22 M | 0.284 / 0.013;  0.1259 / 0.2559 (0.1179 / 0.2397)  1.068 / 1.068
#   c256     65 | 2.53e-06 / 1.21e-06   0.061     0 + 0 of    7.00 M | 0.254 / 0.099;  0.0962 / 0.1807 (0.1064 / 0.1851)  0.904 / 0.976
#   c256    511 | 2.56e-06 / 1.11e-06   0.079    18 + 0 of   55.04 M | 0.231 / 0.090;  0.0918 / 0.1535 (0.0973 / 0.1600)  0.944 / 0.959
#   c256    512 | 2.53e-06 / 1.00e-06   0.067    13 + 1 of   55.15 M | 0.209 / 0.091;  0.0849 / 0.1354 (0.0942 / 0.1575)  0.901 / 0.859
#   c256    515 | 2.53e-06 / 1.12e-06   0.070    13 + 0 of   55.47 M | 0.311 / 0.089;  0.0909 / 0.1383 (0.1034 / 0.1476)  0.879 / 0.937
#   c256   1031 | 2.68e-06 / 1.14e-06   0.078    23 + 3 of  111.05 M | 0.282 / 0.091;  0.0847 / 0.1618 (0.0961 / 0.1914)  0.881 / 0.845
#   c256   4096 | 4.09e-06 / 1.64e-06   0.085   115 + 4 of  441.19 M | 0.228 / 0.090;  0.0921 / 0.1511 (0.1008 / 0.1596)  0.914 / 0.947
#   c128      1 | 3.36e-06 / 1.48e-06   0.052     0 + 0 of    0.08 M | 0.502 / 0.065;  0.1350 / 0.4537 (0.1609 / 0.3518)  0.839 / 1.289
#   c128      2 | 2.30e-06 / 1.45e-06   0.045     0 + 0 of    0.15 M | 0.257 / 0.000;  0.1286 / 0.1733 (0.1546 / 0.2736)  0.832 / 0.633
#   c128     65 | 1.95e-06 / 1.09e-06   0.063     1 + 0 of    4.97 M | 0.464 / 0.127;  0.1089 / 0.1514 (0.1223 / 0.1811)  0.890 / 0.836
#   c128    511 | 2.37e-06 / 1.05e-06   0.067    10 + 1 of   39.08 M | 0.316 / 0.128;  0.1194 / 0.2266 (0.1275 / 0.1834)  0.936 / 1.236
#   c128    512 | 2.00e-06 / 9.63e-07   0.067    14 + 1 of   39.15 M | 0.357 / 0.132;  0.1073 / 0.1735 (0.1158 / 0.1902)  0.927 / 0.912
#   c128    515 | 2.01e-06 / 1.06e-06   0.077     8 + 1 of   39.38 M | 0.381 / 0.130;  0.1204 / 0.2013 (0.1308 / 0.2025)  0.920 / 0.994
#   c128   1031 | 2.74e-06 / 1.02e-06   0.074    18 + 1 of   78.84 M | 0.331 / 0.136;  0.1094 / 0.1633 (0.1253 / 0.1765)  0.873 / 0.925
#   c128   4096 | 4.50e-06 / 1.49e-06   0.080    62 + 0 of  313.23 M | 0.323 / 0.130;  0.1242 / 0.1787 (0.1337 / 0.1845)  0.929 / 0.968
#   c96       1 | 3.03e-06 / 1.20e-06   0.032     0 + 0 of    0.04 M | 0.357 / 0.000;  0.1159 / 0.2041 (0.1025 / 0.1832)  1.131 / 1.114
#   c96       2 | 2.39e-06 / 1.07e-06   0.042     0 + 0 of    0.08 M | 0.132 / 0.088;  0.1452 / 0.2367 (0.1583 / 0.4420)  0.918 / 0.536
#   c96      65 | 1.53e-06 / 8.66e-07   0.046     0 + 0 of    2.60 M | 0.218 / 0.039;  0.0853 / 0.2978 (0.0899 / 0.2777)  0.949 / 1.072
#   c96     511 | 1.89e-06 / 8.29e-07   0.065     5 + 0 of   20.42 M | 0.123 / 0.055;  0.0834 / 0.1938 (0.1031 / 0.2170)  0.809 / 0.893
#   c96     512 | 1.64e-06 / 7.47e-07   0.061     2 + 0 of   20.46 M | 0.150 / 0.047;  0.0710 / 0.1538 (0.0955 / 0.1860)  0.743 / 0.827
#   c96     515 | 1.99e-06 / 7.90e-07   0.064     1 + 0 of   20.58 M | 0.145 / 0.049;  0.0978 / 0.1530 (0.0995 / 0.1615)  0.983 / 0.947
#   c96    1031 | 1.97e-06 / 8.11e-07   0.070     8 + 0 of   41.19 M | 0.133 / 0.054;  0.0830 / 0.1750 (0.1055 / 0.2264)  0.787 / 0.773
# Every followed decision was a tie by the conditions above; the sign of fma(y, scale, shift) differed from the unfused multiply
# and add in 0 or 1 elements per layer (c256 at 515 and 1031, c128 at 65 and 1031), never in the stem or the policy head.  The worst
# gradient quotient (c128, one board: 1.289, blocks.1.se_fc1.bias) is a batch of 81 BatchNorm samples.  fp32 eval outputs: at most
# 0.003 of the tolerance.  Running statistics at 515 boards: worst at 0.043 of rtol 1e-5 / atol 1e-7.
def _fp32_train(c):
    outs, grads, sv, routes = _engine(c, torch.float32, True)
    assert routes["conv"] == 1 + 4 * c.nb and routes["wgrad_tiled"] == 1 + 2 * c.nb, routes
    assert sum(routes[k] for k in ROUTES if k not in ("conv", "wgrad_tiled")) == 0, routes      # fp32: the exact-f32 generic forms only
    relu, sets, order = _decisions(c, sv)
    n_relu, n_pool, total = _check_ties(c, relu, sets)
    ref, ref_grads = _oracle(c, torch.float64, True, True, relu_masks=relu, pool_winners=sets)
    o = max(_close(a, b) for a, b in zip(outs, ref))
    errs = _grad_errs(grads, ref_grads)
    assert set(errs) and set(grads) >= set(ref_grads)
    ratio = max(e[0] for e in errs.values())
    l2 = sorted((e[1], n) for n, e in errs.items())
    print(f"  {c.tower} B={c.B} fp32 train: outputs {o:.3f} of the tolerance; gradients norm {ratio:.2e}, rel L2 worst {l2[-1][0]:.2e} "
          f"({l2[-1][1]}) median {l2[len(l2) // 2][0]:.2e}; followed {n_relu} ReLU + {n_pool} amax decisions of {total}; "
          f"sign depends on fusing the multiply-add: {order}")
    assert all(bool(torch.isfinite(t).all()) for t in outs)
    assert o <= 1.0, (c.tower, c.B, o)
    assert ratio <= FP32_TOL and l2[-1][0] <= FP32_TOL, (c.tower, c.B, ratio, l2[-3:])


def _fp32_eval(c):
    outs, _, _, routes = _engine(c, torch.float32, False, backward=False)
    assert routes["conv"] == 1 + 2 * c.nb and sum(routes.values()) == routes["conv"], routes
    o = [_close(a, b) for a, b in zip(outs, c.ref_eval)]
    print(f"  {c.tower} B={c.B} fp32 eval: policy / value / score at {o[0]:.3f} / {o[1]:.3f} / {o[2]:.3f} of the tolerance")
    assert all(bool(torch.isfinite(t).all()) for t in outs) and max(o) <= 1.0, (c.tower, c.B, o)


def _rel(a, b, ref):
    return float((a.double() - b.double()).norm() / ref.double().norm())


def _bf16_forward(label, c, outs, train):
    """the engine against the bf16-storage emulation and both against fp64, policy logits, relative L2"""
    ref = c.ref_train if train else c.ref_eval
    emu = _emulation(c, train)
    d_emu, d_64, e_64 = _rel(outs[0], emu[0], ref[0]), _rel(outs[0], ref[0], ref[0]), _rel(emu[0], ref[0], ref[0])
    print(f"  {label} {'train' if train else 'eval'}: policy rel L2 hip-emulation {d_emu:.2e}, emulation-fp64 {e_64:.2e} (quotient "
          f"{d_emu / e_64:.3f}), hip-fp64 {d_64:.2e}; value max |hip - emulation| {float((outs[1].double() - emu[1]).abs().max()):.2e}")
    assert all(bool(torch.isfinite(t).all()) for t in outs)
    assert d_emu <= EMU_FACTOR * e_64, (label, train, d_emu, e_64)


def _bf16_gradients(label, c, grads):
    errs = _grad_errs(grads, c.ref_grads)
    l2 = sorted((e[1], n) for n, e in errs.items())
    med, worst = l2[len(l2) // 2][0], l2[-1][0]
    y_med, y_worst = _yardstick(c)
    print(f"  {label} gradients vs fp64: rel L2 median {med:.4f} worst {worst:.4f} ({l2[-1][1]}); oracle under autocast: median "
          f"{y_med:.4f} worst {y_worst:.4f}; quotients {med / y_med:.3f} / {worst / y_worst:.3f}")
    assert med <= MED_FACTOR * y_med and worst <= WORST_FACTOR * y_worst, (label, med, y_med, worst, y_worst)


def _gate_form(c):
    """does the engine's backward take the form without dz (the queries it asks itself)?"""
    Hse = c.m.blocks[0].se_fc1.weight.shape[0]
    return (bool(_lib.query("ka_block_dx_tail_bwd_supported", c.C, Hse, _lib.DTYPE_BF16))
            and bool(_lib.query("ka_conv3x3_dgrad_gated_supported", c.B, c.C, c.C, _lib.DTYPE_BF16, 1)))


def _bf16(c):
    label = f"{c.tower} B={c.B} bf16"
    outs, grads, sv, routes = _engine(c, torch.bfloat16, True)
    print(f"  {label}: routes {routes}, gate form {_gate_form(c)}")
    nb, big = c.nb, c.B >= 512
    if c.tower == "c256" and big:
        # forward convolutions and conv1's data gradient with square 80 inside; conv2's masked data gradient with the corner launch
        assert routes["pc2_corner_in"] == 3 * nb and routes["pc2_corner_out"] == nb and routes["corner"] == nb, routes
        assert routes["conv"] == 1 and routes["pc"] == 0 and routes["pc2"] == 0, routes
    elif c.tower == "c128" and big:
        assert routes["pc2"] == 4 * nb and routes["conv"] == 1, routes
        assert routes["pc"] + routes["pc2_corner_in"] + routes["pc2_corner_out"] + routes["corner"] == 0, routes
    else:
        assert routes["conv"] == 1 + 4 * nb and sum(routes[k] for k in ROUTES[1:6]) == 0, routes
    assert routes["wgrad_lean"] == 1 + 2 * nb and routes["wgrad_tiled"] == 0, routes
    assert _gate_form(c) == (c.tower in ("c256", "c128") and big)
    _bf16_forward(label, c, outs, True)
    outs_e, _, _, routes_e = _engine(c, torch.bfloat16, False, backward=False)
    assert (routes_e["conv"] == 1) == (c.tower != "c96" and big), routes_e
    _bf16_forward(label, c, outs_e, False)
    _bf16_gradients(label, c, grads)


@pytest.mark.parametrize("mode", ["fp32_train", "fp32_eval", "bf16"])
@pytest.mark.parametrize("tower,B", CASES)
def test_engine_against_fp64_oracle(tower, B, mode):
    print(f"\n{tower} B={B} {mode}")
    c = _case(tower, B)
    {"fp32_train": _fp32_train, "fp32_eval": _fp32_eval, "bf16": _bf16}[mode](c)
    if B == 4096:
        print(f"  peak device memory so far {torch.cuda.max_memory_allocated() / 2 ** 30:.1f} GiB")


def test_running_statistics_at_515_boards():
    """c128, 515 boards, momentum 0.1: running mean / variance / num_batches_tracked after one training forward against the fp64
    oracle: the partial-row reduce over 515 boards and the count n = 515 * 81 behind the mean, the variance and n / (n - 1).
    rtol 1e-5; atol 1e-7 is one fp32 rounding of the O(1) terms the stored fp32 value is the sum of."""
    tower, B = "c128", 515
    m = _model(tower, momentum=0.1)
    obs = orc.board_like_obs(B, seed=B).to(DEV)
    with torch.no_grad():
        SEResNetEngine(m).forward(obs, True, False, torch.float32)
    torch.cuda.synchronize()
    ref = {k: (v.to(DEV, torch.float64) if v.dtype.is_floating_point else v.to(DEV)) for k, v in orc.init_like_state_dict(TOWERS[tower]).items()}
    with torch.no_grad(), torch.backends.cudnn.flags(enabled=False):
        orc.seresnet_forward(ref, obs.double(), TOWERS[tower].num_blocks, True, momentum=0.1, update_running=True)
    got, worst, n = m.state_dict(), 0.0, 0
    for k, r in ref.items():
        if "running_" in k:
            n += 1
            worst = max(worst, float(((got[k].double() - r).abs() / (1e-7 + 1e-5 * r.abs())).max()))
            assert torch.allclose(got[k].double(), r, rtol=1e-5, atol=1e-7), (k, float((got[k].double() - r).abs().max()))
        if k.endswith("num_batches_tracked"):
            assert int(got[k]) == int(r) == 1, k
    print(f"\nrunning statistics, {n} tensors: worst at {worst:.3f} of rtol 1e-5 / atol 1e-7")
    assert n == 2 * (2 + 2 * TOWERS[tower].num_blocks)


@pytest.mark.parametrize("T", [torch.float32, torch.bfloat16])
def test_gathered_forward_is_the_forward_of_the_gathered_boards(T):
    """c256, 515 boards picked out of a 1031-board observation tensor: forward(obs, idx=perm) == forward(obs[perm]) bit for bit,
    outputs and gradients."""
    c = _Case()
    c.tower, c.B, c.nb, c.C = "c256", 515, 2, 256
    c.m = _model("c256")
    full = orc.board_like_obs(1031, seed=1031).to(DEV)
    perm = torch.randperm(1031, generator=torch.Generator().manual_seed(515))[:515].to(DEV)
    c.cp, c.cv, c.cs = (t.to(DEV) for t in orc.closed_form_cotangents(515))
    a = _engine(c, T, True, obs=full, idx=perm)
    b = _engine(c, T, True, obs=full[perm].contiguous())
    for x, y in zip(a[0], b[0]):
        assert torch.equal(x, y)
    assert bool((a[0][0] != 0).any())
    for n, g in b[1].items():
        assert torch.equal(a[1][n], g), n


# ------------------------------------------------------------------ route switches at model level (bf16, c256)
# switch -> (environment, environment of the run it must equal bit for bit or None, what the counters must show)
SWITCHES = {
    "KA_CONV_PC2=0": ({"KA_CONV_PC2": "0"}, None),
    "KA_CONV_P=0": ({"KA_CONV_P": "0"}, {"KA_CONV_PC2": "0"}),        # conv3x3_kernel; conv3x3_pc_kernel is bit-identical to it
    "KA_CONV_MT=6": ({"KA_CONV_MT": "6"}, None),
    "KA_CONV_CORNER_IN=0": ({"KA_CONV_CORNER_IN": "0"}, {}),          # the corner launch == the sixth tile inside
    "KA_WGRAD_LEAN=0": ({"KA_WGRAD_LEAN": "0"}, {}),                  # bit-identical slabs
    "KA_TAIL_GATE=0": ({"KA_TAIL_GATE": "0"}, None),
    "KA_DX_TAIL=0": ({"KA_DX_TAIL": "0"}, {"KA_TAIL_GATE": "0"}),     # two launches == ka_block_dx_tail_bwd_du (which forms dz)
}
PYTHON_SIDE = ("KA_TAIL_GATE", "KA_DX_TAIL")


def _with_env(ka_env, monkeypatch, env, c):
    for k in ("KA_CONV_PC2", "KA_CONV_P", "KA_CONV_MT", "KA_CONV_CORNER_IN", "KA_WGRAD_LEAN"):
        ka_env.unset(k)
    for k in PYTHON_SIDE:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        if k in PYTHON_SIDE:
            monkeypatch.setenv(k, v)
        else:
            ka_env.set(k, v)
    return _engine(c, torch.bfloat16, True) + (_gate_form(c),)


@pytest.mark.parametrize("name", list(SWITCHES))
@pytest.mark.parametrize("B", [515, 1031])
def test_route_switch_at_model_level(ka_env, monkeypatch, B, name):
    """Each switch on c256 against the default: the same bf16 bounds, the counters (or the engine's own queries) show that the other
    form ran, and the whole model's outputs and gradients are bit-identical where the kernel tests promise it for the pair."""
    c = _case("c256", B)
    env, same_as = SWITCHES[name]
    base = _with_env(ka_env, monkeypatch, {}, c)
    alt = _with_env(ka_env, monkeypatch, env, c)
    rb, ra = base[3], alt[3]
    print(f"\n{name} B={B}: routes default {rb} gate form {base[4]}\n{' ' * len(name)}        switched {ra} gate form {alt[4]}")
    nb = c.nb
    assert rb["pc2_corner_in"] == 3 * nb and rb["pc2_corner_out"] == nb and rb["corner"] == nb and rb["wgrad_lean"] == 1 + 2 * nb and base[4]
    if name == "KA_CONV_PC2=0":
        # (KA_CONV_P = 1: the producer / consumer kernel takes the forward forms, conv3x3_kernel the data gradients; both leave square 80
        #  to the corner launch)
        assert ra["pc"] == 2 * nb and ra["conv"] == 1 + 2 * nb and ra["corner"] == 4 * nb, ra
        assert ra["pc2_corner_in"] + ra["pc2_corner_out"] == 0 and not alt[4], ra
    elif name == "KA_CONV_P=0":
        assert ra["conv"] == 1 + 4 * nb and ra["corner"] == 4 * nb and ra["pc"] + ra["pc2_corner_in"] + ra["pc2_corner_out"] == 0 and not alt[4], ra
    elif name == "KA_CONV_MT=6":
        assert ra["corner"] == 0 and ra["pc2_corner_in"] + ra["pc2_corner_out"] == 0 and ra["pc"] + ra["conv"] == 1 + 4 * nb and not alt[4], ra
    elif name == "KA_CONV_CORNER_IN=0":
        assert ra["pc2_corner_in"] == 0 and ra["pc2_corner_out"] == 4 * nb and ra["corner"] == 4 * nb and alt[4], ra
    elif name == "KA_WGRAD_LEAN=0":
        assert ra["wgrad_lean"] == 0 and ra["wgrad_tiled"] == 1 + 2 * nb and alt[4], ra
    else:
        # decided in Python: the engine asks the same queries, the environment variable turns the form off; the launches are the default's
        assert ra == rb and alt[4], ra
        assert any(not torch.equal(alt[1][n], g) for n, g in base[1].items()), "the switch changed nothing: gate form not taken?"
    label = f"c256 B={B} bf16 {name}"
    _bf16_forward(label, c, alt[0], True)
    _bf16_gradients(label, c, alt[1])
    if same_as is not None:
        twin = base if same_as == {} else _with_env(ka_env, monkeypatch, same_as, c)
        for x, y in zip(alt[0], twin[0]):
            assert torch.equal(x, y), name
        for n, g in twin[1].items():
            assert torch.equal(alt[1][n], g), (name, n)
