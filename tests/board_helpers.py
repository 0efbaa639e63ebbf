"""Shared by tests/test_board_oracle_cpu.py and tests/test_hip_board_oracle.py: the cases, the float64 references, the
mutants, the error bound and the launch-form rule of the board kernels (csrc/board.hip).  No GPU in here.

Operands are NHWC (B, 81, C), rounded to the case's dtype first; every reference takes those rounded operands (kept as
float64 tensors that hold exactly representable values; per-channel vectors hold float32 values).  The references are
written from the model (oracle/keisei_oracle.py block_forward / global_pool) and the contracts in the comments of board.hip;
test_board_oracle_cpu.py proves each equal to torch autograd in float64.  Run in float32 the SAME formulas give e32 per
output tensor (floored at FLOOR x max|ref|); an fp32 output must lie within MARGIN x e32 of float64, an output stored in
bf16 gets 2**-8 |ref| per element (half a bf16 ulp) on top.  For dse / s1 / s2 of the single-pass tail the fp32 run evaluates
the algebra that kernel documents (sums centred on the BatchNorm mean); the float64 run never does.

Edge planes (EDGE_KINDS) sit on board 1 (C < 9: the ones that do not fit go to board 2) at channels 11 k + 1 mod C: both
halves of a channel pair, different 16-byte pieces.  In the forward case the plane is put into y with scale 1, shift 0, gate
logit 40 (sigmoid exactly 1 in fp32 and fp64), bias 0 and residual 0, so `out` IS the plane whichever operands are given.

Mutants: every reference takes `mutant=`, one wrong line each (MUTANTS maps a name to the references that carry it)."""
import functools
import math
from typing import Optional

import torch

from update_head_helpers import FLOOR, MARGIN, e32_of

BOARD = 81
F64, F32 = torch.float64, torch.float32
DT = {"f32": torch.float32, "bf16": torch.bfloat16}
CODE = {"f32": 0, "bf16": 1}
B = 3
MASK_MARGIN = 2.0 ** -18
EDGE_KINDS = ("max80", "max0", "zero", "const", "ties2", "ties40", "ties80", "allneg")
EDGE_TIES = {"max80": 1, "max0": 1, "zero": 81, "const": 81, "ties2": 2, "ties40": 40, "ties80": 80, "allneg": 1}


# ------------------------------------------------------------------------------------------------ the bound


def bound_of(ref64: torch.Tensor, e32: float, stored: torch.dtype) -> torch.Tensor:
    b = torch.full_like(ref64, MARGIN * e32)
    return b + 2.0 ** -8 * ref64.abs() if stored == torch.bfloat16 else b


def ratio(got: torch.Tensor, ref64: torch.Tensor, e32: float, stored: torch.dtype = torch.float32) -> float:
    """max |got - ref64| / bound: a result passes when this is <= 1 (inf for a non-finite or unwritten element)."""
    got = got.detach().double().cpu().reshape(ref64.shape)
    if not bool(torch.isfinite(got).all()):
        return math.inf
    err = (got - ref64).abs()
    r = torch.where(err == 0, torch.zeros_like(err), err / bound_of(ref64, e32, stored))
    return float(r.max()) if r.numel() else 0.0


def judge(got: dict, ref64: dict, ref32: dict, stored: dict, exact=(), e32: Optional[dict] = None) -> dict:
    """name -> ratio for every tensor of `got`; names in `exact` must be equal to the bit (ratio 0 or inf); e32: the fp32
    run's error per tensor where it is not the one of ref32 itself"""
    out = {}
    for k, g in got.items():
        r64 = ref64[k].double()
        if k in exact:
            out[k] = 0.0 if torch.equal(g.detach().double().cpu().reshape(r64.shape), r64) else math.inf
        else:
            out[k] = ratio(g, r64, e32[k] if e32 else e32_of(ref32[k].double(), r64), stored.get(k, torch.float32))
    return out


def store(t: torch.Tensor, dt: torch.dtype) -> torch.Tensor:
    """a float64 result as the kernel would leave it in memory"""
    return t.to(dt).double()


def ulps32(got: torch.Tensor, ref64: torch.Tensor) -> float:
    """max distance in float32 ulps of the reference's binade (for outputs that are one rounding of a float64 value)"""
    r = ref64.double()
    ulp = torch.where(r == 0, torch.full_like(r, 2.0 ** -149), 2.0 ** (torch.floor(torch.log2(r.abs().clamp_min(2.0 ** -126))) - 23))
    d = (got.detach().double().cpu().reshape(r.shape) - r).abs() / ulp
    return float(d.max()) if bool(torch.isfinite(d).all()) else math.inf


# ------------------------------------------------------------------------------------------------ the form rule


def board16_plan(C: int, dtn: str):
    p16 = 8 if dtn == "bf16" else 4
    if C <= 0 or C % p16:
        return None
    groups = C // p16
    nt = 512 if groups >= 32 else 256
    if groups > nt or nt % groups:
        return None
    return nt, -(-BOARD // (nt // groups))


def pair_form(C: int):
    if not (C >= 2 and C % 2 == 0 and ((C // 2) % 128 == 0 if C // 2 >= 128 else 256 // (C // 2) >= 2)):
        return None
    pairs = C // 2
    cpw = min(pairs, 128)
    ph = min(256 // cpw, BOARD)
    return ("pair", 256, -(-BOARD // ph), pairs // cpw)


def _nrow(C, dtn, nt):
    groups = C // (8 if dtn == "bf16" else 4)
    return nt // max(groups, 64)


def tail_fused_plan(C: int, H: int, dtn: str):
    p = board16_plan(C, dtn)
    if p is None or H <= 0 or H > p[0] or p[0] % H:
        return None
    return p


def board_form(kernel: int, C: int, H: int, dtn: str, pairs: bool = False, p4: bool = True):
    """Mirror of ka_board_form, as a tuple: ("pair", threads, squares per thread, passes) or ("p16", threads, squares per
    thread, "pre" | "rolled" | None, batched, half-width); None = no form covers the shape."""
    if kernel in (0, 1):
        p = None if pairs else board16_plan(C, dtn)
        if kernel == 1 and p:
            return ("p16", p[0], p[1], None, False, False)
        if kernel == 0 and p and p[1] <= 11 and 4 * _nrow(C, dtn, p[0]) * C * 4 <= 65536:
            return ("p16", p[0], 6 if p[1] <= 6 else 11, None, False, False)
        return pair_form(C)
    p = tail_fused_plan(C, H, dtn)
    if p is None or p[1] > (11 if kernel == 2 or dtn == "f32" else 6):
        return None
    nt, nsq = p
    half = (kernel == 4 and p4 and dtn == "bf16" and nt == 512 and C % 4 == 0 and C // 4 <= 512 and 512 % (C // 4) == 0
            and -(-BOARD // (512 // (C // 4))) <= 11 and 512 % H == 0)
    pre = -(-2 * C // (nt // H)) <= 16 and H <= 16
    return ("p16", nt, 11 if half or nsq > 6 else 6, "pre" if pre else "rolled", kernel == 4 and H % 4 == 0, half)


def encode_form(f):
    """board_form's tuple -> the integer ka_board_form returns"""
    if f is None:
        return 0
    if f[0] == "pair":
        return f[1] + 1024 * f[2] + (f[3] << 20)
    flags = 1 | (2 if f[3] == "pre" else 0) | (4 if f[4] else 0) | (8 if f[5] else 0)
    return f[1] + 1024 * f[2] + 65536 * flags


def fwd_se_supported(C: int, H: int, dtn: str, pairs: bool = False) -> bool:
    p = None if pairs else board16_plan(C, dtn)
    if p is None or p[1] > 11 or H <= 0 or H > 16 or p[0] % H:
        return False
    nt, nrow, parts = p[0], _nrow(C, dtn, p[0]), p[0] // H
    return C % parts == 0 and C // parts <= 8 and 2 * C <= nt and 3 * C + nt + H <= 2 * nrow * C and 16 * nrow * C <= 65536


def tail_fused_supported(C, H, dtn) -> bool:
    return board_form(2, C, H, dtn) is not None


def block_dx_tail_supported(C, H, dtn) -> bool:
    return board_form(3, C, H, dtn) is not None


def tail_bwd_lds_bytes(C, H, dtn, dx: bool) -> int:
    nt = tail_fused_plan(C, H, dtn)[0]
    return 4 * (3 * _nrow(C, dtn, nt) * C + 2 * C + nt + H + 3 * C + (5 * C if dx else 0))


# the cases of the activation kernels: (C, dtype, KA_BOARD_PAIRS) -> the form the forward tail / pool is meant to run
FWD_CASES = {
    (32, "bf16", False): ("p16", 256, 6), (64, "bf16", False): ("p16", 256, 6), (128, "bf16", False): ("p16", 256, 6),
    (256, "bf16", False): ("p16", 512, 6), (512, "bf16", False): ("p16", 512, 11),
    (16, "f32", False): ("p16", 256, 6), (64, "f32", False): ("p16", 256, 6), (128, "f32", False): ("p16", 512, 6),
    (256, "f32", False): ("p16", 512, 11),
    (6, "bf16", False): ("pair", 256, 1, 1), (48, "bf16", False): ("pair", 256, 9, 1), (96, "bf16", False): ("pair", 256, 17, 1),
    (6, "f32", False): ("pair", 256, 1, 1), (48, "f32", False): ("pair", 256, 9, 1), (96, "f32", False): ("pair", 256, 17, 1),
    (512, "f32", False): ("pair", 256, 41, 2), (512, "bf16", True): ("pair", 256, 41, 2), (512, "f32", True): ("pair", 256, 41, 2),
    (256, "bf16", True): ("pair", 256, 41, 1), (256, "f32", True): ("pair", 256, 41, 1),
}
PAIR_KERNEL_C = (6, 32, 96, 256, 512)             # ka_tail_bwd_reduce / ka_tail_bwd_dz (channel-pair kernels at every C)
RELU_BN_C = (6, 96, 128, 512)
# (C, H) -> {dtype: (threads, squares, FC loops)} of ka_tail_bwd_fused; a dtype that is missing is not supported
TAIL_CASES = {
    (32, 4): {"bf16": (256, 6, "pre"), "f32": (256, 6, "pre")},
    (64, 2): {"bf16": (256, 6, "pre"), "f32": (256, 6, "pre")},
    (128, 8): {"bf16": (256, 6, "pre"), "f32": (512, 6, "pre")},
    (256, 16): {"bf16": (512, 6, "pre"), "f32": (512, 11, "pre")},
    (256, 32): {"bf16": (512, 6, "rolled"), "f32": (512, 11, "rolled")},
    (512, 16): {"bf16": (512, 11, "rolled")},
    (512, 64): {"bf16": (512, 11, "rolled")},
}
SE_H = (1, 2, 4, 8, 16, 32)
ACT_C = {"bf16": (32, 64, 128, 256, 512, 6, 48, 96), "f32": (16, 64, 128, 256, 6, 48, 96, 512)}


# ------------------------------------------------------------------------------------------------ the data


def q(t: torch.Tensor, dtn: str) -> torch.Tensor:
    return t.to(DT[dtn]).double()


def f32(t: torch.Tensor) -> torch.Tensor:
    return t.float().double()


def edge_plane(kind: str, g: torch.Generator) -> torch.Tensor:
    """81 values, exact in bf16 (sixteenths below 1, and 0.75 / 1.5 / 2.0)"""
    base = torch.randint(1, 16, (BOARD,), generator=g).double() / 16.0
    p = torch.zeros(BOARD, dtype=F64)
    if kind == "max80":
        p[80] = 1.5
    elif kind == "max0":
        p[0] = 1.5
    elif kind == "const":
        p[:] = 0.75
    elif kind == "ties2":
        p = base; p[7] = 2.0; p[80] = 2.0
    elif kind == "ties40":
        p = base; p[0:80:2] = 2.0
    elif kind == "ties80":
        p[:] = 2.0; p[41] = 0.5
    elif kind == "allneg":
        p = -0.5 - base; p[80] = -0.25              # (its maximum, negative, on square 80)
    return p


def edge_slots(C: int):
    """kind -> (board, channel)"""
    slots = {}
    for k, kind in enumerate(EDGE_KINDS):
        slots[kind] = (1, (11 * k + 1) % C) if C >= 16 else (1 + k // C, (k * 5 + 1) % C)
    assert len(set(slots.values())) == len(EDGE_KINDS)
    return slots


def _signed(shape, g, lo=1.0, hi=8.0):
    return (torch.rand(shape, generator=g) * (hi - lo) + lo) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)


@functools.lru_cache(maxsize=None)
def act_case(C: int, dtn: str, H: int = 0, nb: int = B) -> dict:
    """Every operand of the activation kernels for one (C, dtype, H), float64 CPU tensors holding the rounded values."""
    g = torch.Generator().manual_seed(7919 * C + 31 * H + (dtn == "bf16"))
    A = lambda s=1.0, m=0.0: q(torch.randn(nb, BOARD, C, generator=g) * s + m, dtn)
    c = {"C": C, "H": H, "dtn": dtn, "B": nb}
    c["y"], c["res"], c["x"] = A(1.5, 0.3), q(torch.relu(torch.randn(nb, BOARD, C, generator=g)), dtn), q(torch.relu(torch.randn(nb, BOARD, C, generator=g)), dtn)
    c["dout"], c["dxc"], c["dout_up"], c["out_up"] = A(), A(), A(), torch.relu(A())      # out_up: a block output, exact zeros
    for k, s, m in (("scale", 1.0, 0.5), ("invstd", 1.0, 0.5)):
        c[k] = f32(torch.rand(C, generator=g) * s + m)
    c["shift"], c["mean"] = f32(0.3 * torch.randn(C, generator=g)), f32(0.3 + 0.1 * torch.randn(C, generator=g))
    c["se"], c["se_bwd"] = f32(torch.randn(nb, 2 * C, generator=g)), f32(torch.randn(nb, 2 * C, generator=g))
    c["dsq"], c["dpool"] = f32(_signed((nb, C), g)), f32(_signed((nb, 3 * C), g))
    c["slots"] = slots = edge_slots(C) if nb >= 3 else {}
    for kind, (b, ch) in slots.items():
        plane = edge_plane(kind, g)
        c["x"][b, :, ch] = plane
        c["y"][b, :, ch] = plane
        c["res"][b, :, ch] = 0.0
        c["scale"][ch], c["shift"][ch] = 1.0, 0.0
        c["se"][b, ch], c["se"][b, C + ch] = 40.0, 0.0
    c["du_up"] = torch.where(c["out_up"] > 0, c["dout_up"], torch.zeros_like(c["dout_up"]))
    c["bsum"] = f32(c["y"].sum(1))
    c["xpool"] = f32(ref_pool(c["x"], F64))
    if H:
        c["W1"], c["b1"] = f32(torch.randn(H, C, generator=g) / C ** 0.5), f32(torch.randn(H, generator=g))
        c["W2"], c["b2"] = f32(torch.randn(2 * C, H, generator=g) / H ** 0.5), f32(torch.randn(2 * C, generator=g))
        se1 = torch.relu(torch.randn(nb, H, generator=g)) + 0.0
        se1[:, 0] = 0.0                                    # an exact zero on every board: the dh mask is > 0, not >= 0
        if H == 1:
            se1[nb - 1, 0] = 0.5
        c["se1"] = f32(se1)
    return c


PER_BOARD = ("y", "res", "x", "dout", "dxc", "dout_up", "out_up", "du_up", "se", "se_bwd", "dsq", "dpool", "bsum", "xpool", "se1")


def first_board(c: dict) -> dict:
    """board 0 of a case as a case of its own"""
    r = {k: (v[:1].clone() if k in PER_BOARD else v) for k, v in c.items()}
    r["B"], r["slots"] = 1, {}
    return r


@functools.lru_cache(maxsize=None)
def relu_case(C: int, dtn: str) -> dict:
    """ka_relu_bn_bwd_reduce / ka_bn_bwd_apply: the one kernel that recomputes its mask.  Channel `cz` has scale 2, shift -1
    and y = 0.5 on squares 0, 40 and 80 of every board: exact zeros the kernel must mask.  The first salt whose every other
    argument keeps MASK_MARGIN (|scale y| + |shift|) from zero is taken."""
    for salt in range(16):
        g = torch.Generator().manual_seed(104729 * C + 2 * salt + (dtn == "bf16"))
        c = {"C": C, "dtn": dtn, "B": B, "salt": salt}
        c["y"] = q(torch.randn(B, BOARD, C, generator=g) * 1.5 + 0.3, dtn)
        c["dh"], c["dz"] = q(torch.randn(B, BOARD, C, generator=g), dtn), q(torch.randn(B, BOARD, C, generator=g), dtn)
        c["scale"], c["shift"] = f32(torch.rand(C, generator=g) + 0.5), f32(0.3 * torch.randn(C, generator=g))
        c["mean"], c["invstd"] = f32(0.3 + 0.1 * torch.randn(C, generator=g)), f32(torch.rand(C, generator=g) + 0.5)
        c["k"] = f32(torch.cat([torch.rand(C, generator=g) + 0.5, _signed((C,), g, 0.05, 0.2), _signed((C,), g, 0.05, 0.2)]))
        cz = c["cz"] = (C // 2 + 1) % C
        c["scale"][cz], c["shift"][cz] = 2.0, -1.0
        c["y"][:, [0, 40, 80], cz] = 0.5
        if relu_margin_ok(c):
            return c
    raise AssertionError(f"no salt keeps the ReLU margin at C={C} {dtn}")


def relu_margin_ok(c: dict) -> bool:
    sy, sh = c["y"] * c["scale"], c["shift"]
    arg = sy + sh
    placed = torch.zeros_like(arg, dtype=torch.bool)
    placed[:, [0, 40, 80], c["cz"]] = True
    ok_placed = bool((arg[placed] == 0).all())
    return ok_placed and bool((arg[~placed].abs() >= MASK_MARGIN * (sy.abs() + sh.abs())[~placed]).all())


# ------------------------------------------------------------------------------------------------ the references


def _S(t: torch.Tensor, mutant) -> torch.Tensor:
    """sum over the 81 squares (mutant sq80_twice: a lane past the board adds square 80 again)"""
    s = t.sum(1)
    return s + t[:, 80] if mutant == "sq80_twice" else s


def _rows(t: torch.Tensor, mutant) -> torch.Tensor:
    """a per-board row (mutant board_row: board b reads board b - 1's row)"""
    return t.roll(1, 0) if mutant == "board_row" else t


def ref_tail_fwd(c, dt, use_se=True, use_res=True, se=None, mutant=None) -> torch.Tensor:
    """out = relu((scale y + shift) sigmoid(a) + b + res)        (se_resnet.py:83-90)"""
    C = c["C"]
    v = c["y"].to(dt) * c["scale"].to(dt) + c["shift"].to(dt)
    if use_se:
        s = _rows((c["se"] if se is None else se).to(dt), mutant)
        v = v * torch.sigmoid(s[:, None, :C]) + s[:, None, C:]
    if use_res:
        v = v + c["res"].to(dt)
    return torch.relu(v)


def ref_pool(x: torch.Tensor, dt, mutant=None) -> torch.Tensor:
    """[mean | max | std (correction 0) | ties] of (B, 81, C) -> (B, 4C)         (keisei_oracle.global_pool + the tie count)"""
    x = x.to(dt)
    xx = torch.cat([x, x[:, 80:]], 1) if mutant == "sq80_twice" else x
    mean = xx.sum(1) / BOARD
    mx = x.amax(1)
    var = ((xx - mean[:, None]) ** 2).sum(1) / (BOARD - 1 if mutant == "std_corr1" else BOARD)
    ties = (xx == mx[:, None]).sum(1).to(dt)
    return torch.cat([mean, mx, var.sqrt(), ties], 1)


def ref_se_chain(c, dt, bias=True, mutant=None) -> dict:
    """sqz = scale bsum / 81 + shift, se1 = relu(W1 sqz + b1), se = W2 se1 + b2          (se_resnet.py:83-86)"""
    z = c["scale"].to(dt) * (_rows(c["bsum"].to(dt), mutant) / BOARD) + c["shift"].to(dt)
    h = z @ c["W1"].to(dt).t() + (c["b1"].to(dt) if bias else 0.0)
    h = torch.relu(h)
    se = h @ c["W2"].to(dt).t() + (c["b2"].to(dt) if bias else 0.0)
    return {"sqz": z, "se1": h, "se": se}


def ref_tail_bwd(c, dt, dout=None, out=None, dsq=None, fused_algebra=False, mutant=None) -> dict:
    """Backward of out = relu(z sigmoid(a) + b + res), z = scale y + shift, and of the SE chain behind a / b:
    du = dout [out > 0]; dse = [sig'(a) sum du z | sum du]; dh = [se1 > 0] dse W2; dsq = dh W1; dz = du sig(a) + dsq / 81;
    s1 = sum dz, s2 = sum dz yhat.  `dsq` given: the two-launch path (ka_tail_bwd_dz takes it as an operand)."""
    C = c["C"]
    dout = (c["dout"] if dout is None else dout).to(dt)
    out = (c["x"] if out is None else out).to(dt)
    y, scale, shift, mean, invstd = (c[k].to(dt) for k in ("y", "scale", "shift", "mean", "invstd"))
    du = dout * ((out >= 0) if mutant == "mask_ge" else (out > 0))
    sig = torch.sigmoid(_rows(c["se_bwd"].to(dt), mutant)[:, :C])
    Sg = _S(du, mutant)
    if fused_algebra:                                  # board.hip, tail_bwd_fused_kernel: sums centred on the BatchNorm mean
        yc = y - mean
        Sgy, Sy = _S(du * yc, mutant), _S(yc, mutant)
        duz = scale * Sgy + (shift + mean * scale) * Sg
    else:
        duz = _S(du * (y * scale + shift), mutant)
    dse = torch.cat([duz * (sig if mutant == "sig_not_dsig" else sig * (1 - sig)), Sg], 1)
    r = {"du": du, "dse": dse}
    if dsq is None:
        dh = dse @ c["W2"].to(dt)
        if mutant != "dh_mask":
            dh = dh * (c["se1"].to(dt) > 0)
        dsq = dh @ c["W1"].to(dt)
        r["dh"] = dh
    else:
        dsq = dsq.to(dt)
    add = dsq / BOARD
    r["dsq"], r["gate"], r["add"] = dsq, sig, add
    dz = du * sig[:, None] + (0.0 if mutant == "dsq81" else add[:, None])
    r["dz"] = dz
    if fused_algebra:
        r["s1"] = sig * Sg + BOARD * add
        r["s2"] = invstd * (sig * Sgy + (0.0 if mutant == "s2_no_addSy" else add * Sy))
    else:
        yhat = (y - mean) * invstd
        r["s1"] = _S(dz, mutant)
        r["s2"] = _S(du * sig[:, None] * yhat, mutant) if mutant == "s2_no_addSy" else _S(dz * yhat, mutant)
    return r


def ref_block_dx(c, dt, use_dxc=True, up="masked", x=None, mutant=None) -> dict:
    """dx = [dxc] + [dout_up [out_up > 0] | du_up] + backward of [mean | max | std] pooling of x with the saved statistics:
    dpool_mean / 81; dpool_max / ties on every square at the max; dpool_std (x - mean) / (81 std), 0 where std == 0.
    du = dx [x > 0] is what the chain forms write."""
    C = c["C"]
    x = (c["x"] if x is None else x).to(dt)
    xp, dp = c["xpool"].to(dt), _rows(c["dpool"].to(dt), mutant)
    mean, mx, std, ties = xp[:, :C], xp[:, C:2 * C], xp[:, 2 * C:3 * C], xp[:, 3 * C:]
    gm = dp[:, :C] / BOARD
    gx = dp[:, C:2 * C] if mutant in ("max_not_div", "max_first") else dp[:, C:2 * C] / ties
    gs = dp[:, 2 * C:] / (BOARD * std)
    if mutant != "std_nozero":
        gs = torch.where(std > 0, gs, torch.zeros_like(gs))
    at_max = x == mx[:, None]
    if mutant == "max_first":
        at_max = at_max & (at_max.cumsum(1) == 1)
    g = gm[:, None] + gs[:, None] * (x - mean[:, None]) + torch.where(at_max, gx[:, None].expand_as(x), torch.zeros_like(x))
    if use_dxc:
        g = g + c["dxc"].to(dt)
    if up == "masked":
        o = c["out_up"].to(dt)
        g = g + c["dout_up"].to(dt) * ((o >= 0) if mutant == "mask_ge" else (o > 0))
    elif up == "du":
        d = c["du_up"].to(dt)
        g = g + (d * (c["y"].to(dt) > 0) if mutant == "du_up_remask" else d)
    return {"dx": g, "du": g * (x > 0)}


def ref_relu_bn_bwd(c, dt, mutant=None) -> dict:
    """da = dh [scale y + shift > 0], s1 = sum da, s2 = sum da yhat"""
    y = c["y"].to(dt)
    arg = y * c["scale"].to(dt) + c["shift"].to(dt)
    da = c["dh"].to(dt) * ((arg >= 0) if mutant == "mask_ge" else (arg > 0))
    return {"da": da, "s1": _S(da, mutant), "s2": _S(da * ((y - c["mean"].to(dt)) * c["invstd"].to(dt)), mutant)}


def ref_bn_bwd_apply(c, dt, mutant=None) -> dict:
    """dy = k1 dz + k2 + k3 y"""
    C = c["C"]
    k = c["k"].to(dt)
    return {"dy": k[:C] * c["dz"].to(dt) + (0.0 if mutant == "k2" else k[C:2 * C]) + k[2 * C:] * c["y"].to(dt)}


def ref_bn_coeffs(sums, count, gamma, beta, rm, rv, momentum, eps, dt, mutant=None) -> dict:
    """BatchNorm2d in training mode from [sum x | sum x^2]: scale / shift with y_hat gamma + beta == x scale + shift, and
    the running statistics (momentum form, unbiased variance; count 1: the biased one)"""
    C = gamma.numel()
    s = sums.to(dt)
    mean = s[:C] / count
    var = (s[C:] / count - mean * mean).clamp_min(0.0)
    invstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma.to(dt) * invstd
    r = {"scale": scale, "shift": beta.to(dt) - mean * scale, "mean": mean, "invstd": invstd}
    if rm is not None:
        unb = var * count / (count - 1.0) if count > 1 and mutant != "rv_biased" else var
        r["running_mean"] = (1 - momentum) * rm.to(dt) + momentum * mean
        r["running_var"] = (1 - momentum) * rv.to(dt) + momentum * unb
    return r


def ref_bn_bwd_coeffs(sums_local, sums_global, count, gamma, mean, invstd, train, dt, mutant=None) -> dict:
    """dbeta = sum dz, dgamma = sum dz yhat (local sums); dy = k1 dz + k2 + k3 y with k1 = gamma invstd,
    k3 = -gamma invstd^2 S2 / n, k2 = -gamma invstd S1 / n - k3 mean (global sums); eval mode: k2 = k3 = 0"""
    C = gamma.numel()
    l, gl = sums_local.to(dt), sums_global.to(dt)
    g, is_, mu = gamma.to(dt), invstd.to(dt), mean.to(dt)
    on = train or mutant == "eval_k"
    k3 = -g * is_ * is_ * gl[C:] / count if on else torch.zeros_like(g)
    k2 = -g * is_ * gl[:C] / count - k3 * mu if on else torch.zeros_like(g)
    return {"dbeta": l[:C], "dgamma": l[C:], "k": torch.cat([g * is_, k2, k3])}


def ref_bn_eval_coeffs(gamma, beta, rm, rv, eps, dt) -> dict:
    sc = gamma.to(dt) / torch.sqrt(rv.to(dt) + eps)
    return {"scale": sc, "shift": beta.to(dt) - rm.to(dt) * sc}


def ref_affine_rows(x, a, s, mul, dt) -> torch.Tensor:
    return a.to(dt) * (x.to(dt) * mul) + s.to(dt)


def ref_obs_to_nhwc(obs: torch.Tensor, idx, cpad: int) -> torch.Tensor:
    """(S, Cobs, 9, 9) -> (B, 81, Cpad): rows gathered through idx, channels past Cobs zero"""
    o = obs if idx is None else obs[idx]
    out = torch.zeros(o.shape[0], BOARD, cpad, dtype=o.dtype)
    out[:, :, :o.shape[1]] = o.reshape(o.shape[0], o.shape[1], BOARD).permute(0, 2, 1)
    return out


def ref_nhwc_to_nchw(x: torch.Tensor) -> torch.Tensor:
    return x.permute(0, 2, 1).reshape(x.shape[0], x.shape[2], 9, 9).contiguous()


# mutant -> the references that carry it (and, in the summary of the GPU file, the tests that hold the kernels to them)
MUTANTS = {
    "dsq81": ("tail_bwd",), "k2": ("bn_bwd_apply",), "mask_ge": ("tail_bwd", "block_dx", "relu_bn_bwd"),
    "max_not_div": ("block_dx",), "max_first": ("block_dx",), "std_nozero": ("block_dx",), "sig_not_dsig": ("tail_bwd",),
    "dh_mask": ("tail_bwd",), "std_corr1": ("pool",), "du_up_remask": ("block_dx",), "s2_no_addSy": ("tail_bwd",),
    "rv_biased": ("bn_coeffs",), "eval_k": ("bn_bwd_coeffs",), "sq80_twice": ("pool", "tail_bwd", "relu_bn_bwd"),
    "board_row": ("tail_fwd", "tail_bwd", "block_dx", "se_chain"),
}


# ------------------------------------------------------------------------------------------------ families
# One entry per contract: fn(case, dt, mutant=None, alg=False) -> name -> tensor; `act`: the outputs stored in the activation
# dtype; `exact`: the outputs that must be equal to the bit; `alg`: the fp32 run may take the fused tail's algebra.


def _split_pool(p, C):
    return {"mean": p[:, :C], "max": p[:, C:2 * C], "std": p[:, 2 * C:3 * C], "ties": p[:, 3 * C:]}


def fam_tail_fwd(use_se, use_res):
    return lambda c, dt, mutant=None, alg=False: {"out": ref_tail_fwd(c, dt, use_se, use_res, mutant=mutant)}


def fam_pool(c, dt, mutant=None, alg=False, x=None):
    return _split_pool(ref_pool(c["x"] if x is None else x, dt, mutant), c["C"])


def fam_se_chain(bias):
    return lambda c, dt, mutant=None, alg=False: ref_se_chain(c, dt, bias, mutant)


def fam_tail_fused(c, dt, mutant=None, alg=False, dout=None, out=None):
    r = ref_tail_bwd(c, dt, dout=dout, out=out, fused_algebra=alg, mutant=mutant)
    return {k: r[k] for k in ("dse", "dh", "dz", "s1", "s2", "gate", "add")}


def fam_tail_unfused(c, dt, mutant=None, alg=False):
    r = ref_tail_bwd(c, dt, dsq=c["dsq"], mutant=mutant)
    return {k: r[k] for k in ("dse", "dz", "s1", "s2")}


def fam_block_dx(use_dxc, up):
    def fn(c, dt, mutant=None, alg=False):
        r = ref_block_dx(c, dt, use_dxc, up, mutant=mutant)
        return r if up == "du" else {"dx": r["dx"]}
    return fn


def fam_relu_bn(c, dt, mutant=None, alg=False):
    return ref_relu_bn_bwd(c, dt, mutant)


def fam_bn_apply(c, dt, mutant=None, alg=False):
    return ref_bn_bwd_apply(c, dt, mutant)


def act_cases(kernel_c=None):
    return [(C, dtn) for dtn in ("bf16", "f32") for C in (kernel_c or ACT_C[dtn])]


def tail_cases():
    return [(C, H, dtn) for (C, H), d in TAIL_CASES.items() for dtn in d]


def se_cases():
    return [(C, H, dtn) for dtn in ("bf16", "f32") for C in ACT_C[dtn] for H in SE_H if fwd_se_supported(C, H, dtn)]


FAMILIES = {
    # name: (fn, act outputs, exact outputs, cases -> act_case / relu_case arguments, mutants)
    "tail_fwd": (fam_tail_fwd(True, True), ("out",), (), lambda: act_cases(), ("board_row",)),
    "tail_fwd_nores": (fam_tail_fwd(True, False), ("out",), (), lambda: act_cases(), ("board_row",)),
    "pool": (fam_pool, (), ("max", "ties"), lambda: act_cases(), ("std_corr1", "sq80_twice")),
    "se_chain": (fam_se_chain(True), (), (), se_cases, ("board_row",)),
    "se_chain_nobias": (fam_se_chain(False), (), (), se_cases, ("board_row",)),
    "tail_fused": (fam_tail_fused, ("dz",), (), tail_cases,
                   ("dsq81", "mask_ge", "sig_not_dsig", "dh_mask", "s2_no_addSy", "sq80_twice", "board_row")),
    "tail_unfused": (fam_tail_unfused, ("dz",), (), lambda: act_cases(PAIR_KERNEL_C),
                     ("dsq81", "mask_ge", "sig_not_dsig", "s2_no_addSy", "sq80_twice", "board_row")),
    "block_dx": (fam_block_dx(True, "masked"), ("dx",), (), lambda: act_cases(),
                 ("mask_ge", "max_not_div", "max_first", "std_nozero", "board_row")),
    "block_dx_heads": (fam_block_dx(False, "none"), ("dx",), (), lambda: act_cases(),
                       ("max_not_div", "max_first", "std_nozero", "board_row")),
    "block_dx_du": (fam_block_dx(True, "du"), ("dx", "du"), (), tail_cases,
                    ("max_not_div", "max_first", "std_nozero", "du_up_remask", "board_row")),
    "relu_bn_bwd": (fam_relu_bn, ("da",), (), lambda: act_cases(RELU_BN_C), ("mask_ge", "sq80_twice")),
    "bn_bwd_apply": (fam_bn_apply, ("dy",), (), lambda: act_cases(RELU_BN_C), ("k2",)),
}


def family_case(name: str, args):
    if name in ("relu_bn_bwd", "bn_bwd_apply"):
        return relu_case(*args)
    if len(args) == 3:
        return act_case(args[0], args[2], args[1])
    return act_case(args[0], args[1])


def judge_family(name: str, c: dict, got: dict, alg: bool = False, **kw) -> dict:
    """the ratios of `got` (name -> tensor as stored) against the family's float64 reference"""
    fn, act, exact = FAMILIES[name][:3]
    r64, r32 = fn(c, F64, **kw), fn(c, F32, alg=alg, **kw)
    return judge(got, r64, r32, {k: DT[c["dtn"]] for k in act}, exact)


def as_stored(name: str, c: dict, res: dict) -> dict:
    act = FAMILIES[name][1]
    return {k: store(v, DT[c["dtn"]] if k in act else torch.float32) for k, v in res.items()}
