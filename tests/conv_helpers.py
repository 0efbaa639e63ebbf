"""Shared by tests/test_conv_exact_cpu.py and tests/test_hip_conv_exact.py: integer-valued operands of the 3x3 convolution and
of its fused data gradient, their fp64 references, the kernel forms of csrc/conv3x3.hip with the switches and the route
counters of each, and the case lists.

Why integers: with ternary activations and weights, scale in {-1, 1, 2}, shift and per-board bias in {-1, 0, 1} the transformed
input h = relu(x * scale + shift) + bias is an integer of magnitude <= 4 (exact in bf16), every product h * w is exact, and
every partial sum is an integer below 2^24: fp32 addition of such numbers is exact in ANY order, so the output must equal the
fp64 reference to the bit whatever the chunking, the tap walk, the MFMA grouping or the number of boards per unit, and one
dropped or misplaced product (one tap of one channel of one square) changes it.  Outputs stored as bf16 are kept at or below
256 (every integer up to 256 is a bf16), so the stored value is the integer itself; `check_exact` asserts both conditions for
every case, and the CPU test runs it for all of them.

The references are computed in fp64 and, being integers (or halves) far below 2^24, held as float32 -- `exact32` asserts that
nothing is lost.  A reference is built once for the largest batch of its kind and sliced: boards are independent."""
import functools
from typing import NamedTuple, Optional, Tuple

import torch
import torch.nn.functional as F

from wgrad_helpers import ROUTES, TRANSFORMS, transform64

BOARD = 81
LIMIT = 2 ** 24                                  # below it every integer is an fp32
BF16_INT = 256                                   # up to it every integer is a bf16
B_TRAIN = {256: 1027, 128: 515}                  # the largest training batch of the cases per channel count: every smaller one is a slice
B_SMALL = 5

# every switch conv_dispatch reads (csrc/common.h: KA_OPTIONS); a form sets its own and unsets all the others
SWITCHES = ("KA_CONV_P", "KA_CONV_MT", "KA_CONV_PC2", "KA_CONV_PC2_SKIP", "KA_CONV_PC2_STAG", "KA_CONV_CORNER_IN", "KA_CONV_P_STAG",
            "KA_CONV_P_PRIO", "KA_CONV_P_WGS", "KA_CONV_P_NPW", "KA_CONV_WM", "KA_CONV_KC", "KA_CONV_NTW", "KA_CONV_STAGGER",
            "KA_CONV_PRIO")


# ------------------------------------------------------------------------------------------------ layouts and the oracle
def nchw(t):
    """(B, 81, C) -> (B, C, 9, 9)"""
    B, _, C = t.shape
    return t.reshape(B, 9, 9, C).permute(0, 3, 1, 2)


def nhwc(t):
    """(B, C, 9, 9) -> (B, 81, C), contiguous"""
    B, C = t.shape[:2]
    return t.permute(0, 2, 3, 1).reshape(B, BOARD, C).contiguous()


def conv64(h, w, adjoint):
    """fp64 oracle.  Forward: h (B, 81, Cin), w (Cout, Cin, 3, 3) -> conv2d(h, w, padding 1), (B, 81, Cout).
    Adjoint: h = dy (B, 81, Cin), w (Cin, Cout, 3, 3) -- the weight of the forward layer Cout -> Cin -- -> the gradient of that
    layer's input, (B, 81, Cout)."""
    x, wd = nchw(h.double()), w.double()
    if adjoint:
        y = torch.nn.grad.conv2d_input((x.shape[0], w.shape[1], 9, 9), wd, x, padding=1)
    else:
        y = F.conv2d(x, wd, padding=1)
    return nhwc(y)


def conv_taps64(h, w, adjoint):
    """The same operation written out tap by tap, nine shifted matmuls over a zero-haloed 11 x 11 image -- independent of
    conv2d.  The adjoint is the forward form with the kernel flipped and transposed: tap t multiplies w[c, n, 8 - t], which is
    the convention of ka_pack_conv3x3's mode 1."""
    B, _, Cin = h.shape
    Cout = w.shape[1] if adjoint else w.shape[0]
    img = torch.zeros(B, 11, 11, Cin, dtype=torch.float64)
    img[:, 1:10, 1:10] = h.double().reshape(B, 9, 9, Cin)
    out = torch.zeros(B, 9, 9, Cout, dtype=torch.float64)
    wd = w.double()
    for tap in range(9):
        patch = img[:, tap // 3:tap // 3 + 9, tap % 3:tap % 3 + 9]         # square p + tap
        if adjoint:
            src = 8 - tap
            out += patch @ wd[:, :, src // 3, src % 3]                     # (Cin, Cout)
        else:
            out += patch @ wd[:, :, tap // 3, tap % 3].t()                 # (Cout, Cin)^T
    return out.reshape(B, BOARD, Cout)


def exact32(t):
    """fp64 -> float32, asserting that it is the same number."""
    s = t.float()
    assert torch.equal(s.double(), t), "the reference does not fit float32 exactly"
    return s


def amax(t):
    return float(t.abs().max()) if t.numel() else 0.0


def check_exact(label, Cin, h, w, out, stored=(), board_terms=(), dense=False):
    """The two conditions of the module docstring.  h: the tensor the convolution multiplies; out: its fp64 result; stored: the
    other tensors a bf16 kernel stores (dy_out, x_out); board_terms: (B, 81, C) tensors of which a kernel sums 81 squares in fp32
    beside out and out^2.  dense (the rounding case): outputs may pass 256, and the per-board sums are bounded by what they
    really are instead of by 81 x the maximum."""
    assert 9 * Cin * amax(h) * amax(w) < LIMIT, f"{label}: an accumulator partial sum could reach 2^24"
    terms = [out, out * out, *board_terms]
    for t in terms:
        bound = amax(t.abs().sum(1)) if dense else BOARD * amax(t)
        assert bound < LIMIT, f"{label}: a per-board partial sum could reach 2^24"
    if not dense:
        for t in (out, *stored):
            assert amax(t) <= BF16_INT, f"{label}: max |value| {amax(t)} > 256 is not stored exactly as bf16"
    for t in (h, w, *stored):
        assert torch.equal(t.double(), t.to(torch.bfloat16).double()), f"{label}: an operand is not a bf16"


# ------------------------------------------------------------------------------------------------ operands
def gen(*key):
    seed = 17
    for k in key:
        seed = (seed * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


def pick(g, values, *shape):
    return torch.tensor(values, dtype=torch.float32)[torch.randint(0, len(values), shape, generator=g)]


def ints(g, lim, *shape):
    return torch.randint(-lim, lim + 1, shape, generator=g).float()


def sparse_ternary(g, num, den, *shape):
    """-1 / +1 with probability num / (2 den) each, else 0 (num / den = 2 / 3: uniform over {-1, 0, 1})"""
    keep = torch.randint(0, den, shape, generator=g) < num
    return pick(g, (-1.0, 1.0), *shape) * keep


class Fwd(NamedTuple):
    """A forward-ABI case (ka_conv3x3_fwd / _fwd_keep; adjoint: the same entry on a mode-1 pack).  Cin / Cout are what the
    kernel sees (padded); w holds the real channels only."""
    x: torch.Tensor                              # (B, 81, Cin) float32; padded channels hold data too
    w: torch.Tensor                              # (Cout_real, Cin_real, 3, 3), adjoint: (Cin_real, Cout_real, 3, 3)
    scale: Optional[torch.Tensor]
    shift: Optional[torch.Tensor]
    relu: bool
    bias: Optional[torch.Tensor]                 # (B, Cin)
    adjoint: bool
    h: torch.Tensor                              # (B, 81, Cin) float32 reference of x_out
    out: torch.Tensor                            # (B, 81, Cout) float32 reference; channels past Cout_real are zero
    bsum: torch.Tensor                           # (B, Cout) per-board sums of out
    sq: torch.Tensor                             # (B, Cout) fp64 per-board sums of out^2 (the test sums the boards it ran)


@functools.lru_cache(maxsize=None)
def fwd_data(B, Cin, Cout, transform="plain", num=2, den=3, Cin_real=0, Cout_real=0, adjoint=False, xlim=1) -> Fwd:
    """Ternary x (xlim = 2: -2 .. 2, the rounding case), ternary w of density num / den; must not be modified."""
    Cin_real, Cout_real = Cin_real or Cin, Cout_real or Cout
    affine, relu, with_bias = TRANSFORMS[transform]
    g = gen(1, B, Cin, Cout, list(TRANSFORMS).index(transform), num, den, Cin_real, Cout_real, adjoint, xlim)
    x = ints(g, xlim, B, BOARD, Cin)
    wshape = (Cin_real, Cout_real, 3, 3) if adjoint else (Cout_real, Cin_real, 3, 3)
    w = sparse_ternary(g, num, den, *wshape)
    scale, shift, bias = pick(g, (-1.0, 1.0, 2.0), Cin), ints(g, 1, Cin), ints(g, 1, B, Cin)
    scale, shift, bias = (scale if affine else None), (shift if affine else None), (bias if with_bias else None)
    h = transform64(x, scale, shift, relu, bias)
    out = torch.zeros(B, BOARD, Cout, dtype=torch.float64)
    out[:, :, :Cout_real] = conv64(h[:, :, :Cin_real], w, adjoint)
    if Cin_real < Cin:
        assert amax(h[:, :, Cin_real:]) > 0, "the padded input channels must hold data"
    dense = xlim > 1
    check_exact(f"fwd B{B} {Cin}x{Cout} {transform}", Cin, h, w, out, stored=(h,), dense=dense)
    return Fwd(x, w, scale, shift, relu, bias, adjoint, exact32(h), exact32(out), exact32(out.sum(1)), (out * out).sum(1))


class Dgrad(NamedTuple):
    """A case of ka_conv3x3_dgrad_fused (ga None) or ka_conv3x3_dgrad_fused_gated: dy = dz * k0 + k1 + in2 * k2 with dz = a, or
    a * gate + add; dh = the adjoint convolution of dy; masked: da = bf16(dh) * [ep_scale * y + ep_shift > 0]."""
    a: torch.Tensor                              # (B, 81, Cin): in, or du
    in2: torch.Tensor                            # (B, 81, Cin)
    k: torch.Tensor                              # (3 Cin,)
    ga: Optional[torch.Tensor]                   # (2, B, Cin): gate | add
    y: torch.Tensor                              # (B, 81, Cout)
    ep: Tuple[torch.Tensor, ...]                 # scale, shift, mean, invstd: (Cout,) each
    w: torch.Tensor                              # (Cin, Cout, 3, 3): packed with mode 1
    dy: torch.Tensor                             # references, float32 (sums of the masked form: fp64, per board)
    dh: torch.Tensor
    bsum: torch.Tensor
    da: torch.Tensor
    s1: torch.Tensor
    s2: torch.Tensor


@functools.lru_cache(maxsize=None)
def dgrad_data(B, Cin, Cout, gated=False, num=1, den=4, alim=1, with_k1=True) -> Dgrad:
    g = gen(2, B, Cin, Cout, gated, num, den, alim, with_k1)
    a, in2, y = ints(g, alim, B, BOARD, Cin), ints(g, 1, B, BOARD, Cin), ints(g, 1, B, BOARD, Cout)
    k = torch.cat([pick(g, (-1.0, 1.0), Cin), ints(g, 1, Cin) * float(with_k1), ints(g, 1, Cin)])
    ga = torch.stack([pick(g, (-1.0, 1.0, 2.0), B, Cin), ints(g, 1, B, Cin)]) if gated else None
    ep = (pick(g, (-1.0, 1.0, 2.0), Cout), pick(g, (-0.5, 0.5), Cout), ints(g, 1, Cout), pick(g, (0.5, 1.0, 2.0), Cout))
    w = sparse_ternary(g, num, den, Cin, Cout, 3, 3)
    dz = a.double()
    if gated:
        dz = dz * ga[0].double()[:, None, :] + ga[1].double()[:, None, :]
    kd = k.double()
    dy = dz * kd[:Cin] + kd[Cin:2 * Cin] + in2.double() * kd[2 * Cin:]
    dh = conv64(dy, w, True)
    pre = y.double() * ep[0].double() + ep[1].double()
    assert float(pre.abs().min()) >= 0.5, "the mask must be decided exactly"
    # the masked value is the bf16 the kernel stores, and the two sums are sums of THAT (conv_epilogue, conv_epilogue_masked_pair
    # and the corner epilogues all take `(float)(__bf16)acc`); below 256 the rounding changes nothing
    da = dh.to(torch.bfloat16).double() * (pre > 0)
    t2 = da * (y.double() - ep[2].double()) * ep[3].double()
    dense = alim > 1
    # (the pair epilogue sums da * y and centres afterwards: bounded by the same product)
    check_exact(f"dgrad B{B} {Cin}x{Cout} gated={gated}", Cin, dy, w, dh, stored=(dy,), board_terms=(da, 4.0 * da), dense=dense)
    return Dgrad(a, in2, k, ga, y, ep, w, exact32(dy), exact32(dh), exact32(dh.sum(1)), exact32(da), da.sum(1), t2.sum(1))


def take(d, B):
    """The first B boards of a case (every per-board tensor sliced; the per-channel ones kept)."""
    n = d.x.shape[0] if isinstance(d, Fwd) else d.a.shape[0]
    assert B <= n
    if B == n:
        return d
    cut = {}
    for name, v in d._asdict().items():
        if isinstance(v, torch.Tensor) and name not in ("w", "scale", "shift", "k"):
            cut[name] = v[:, :B].contiguous() if name == "ga" else v[:B]
    return d._replace(**cut)


# ------------------------------------------------------------------------------------------------ failure messages
def explain(label, got, exp, B):
    """What differs between two tensors of shape (B, 81, C) or (B, C): how many elements, the worst (board, square, channel)
    with both values, and whether the differences are confined to square 80, to the last board or pair, to one board of every
    pair, to one 16-channel tile, or to the boards past the first 512 (the second unit of a persistent workgroup)."""
    g, e = got.detach().double().cpu(), exp.detach().double().cpu()
    if g.dim() == 2:
        g, e = g[:, None, :], e[:, None, :]
    bad = ~(g == e)
    if not bool(bad.any()):
        return f"{label}: equal"
    diff = (g - e).abs().nan_to_num(nan=float("inf"), posinf=float("inf"))
    diff[~bad] = 0
    b, p, c = (int(v) for v in torch.unravel_index(diff.argmax(), diff.shape))
    boards = torch.nonzero(bad.any(2).any(1)).flatten().tolist()
    squares = torch.nonzero(bad.any(2).any(0)).flatten().tolist()
    tiles = sorted({int(v) // 16 for v in torch.nonzero(bad.any(1).any(0)).flatten().tolist()})
    notes = []
    if g.shape[1] == BOARD and squares == [80]:
        notes.append("confined to square 80")
    if boards == [B - 1]:
        notes.append("confined to the last board")
    elif min(boards) >= 2 * ((B - 1) // 2):
        notes.append("confined to the last pair")
    if len(boards) > 1 and len({b % 2 for b in boards}) == 1:
        notes.append(f"confined to the {'second' if boards[0] % 2 else 'first'} board of the pairs")
    if len(tiles) == 1:
        notes.append(f"confined to the 16-channel tile {tiles[0]}")
    if min(boards) >= 512:
        notes.append("confined to the boards past the first 512 (a workgroup's second unit)")
    return (f"{label}: {int(bad.sum())} of {bad.numel()} elements differ on {len(boards)} boards (first {boards[:6]}), squares "
            f"{squares[:12]}{'...' if len(squares) > 12 else ''}, channel tiles {tiles[:12]}; worst (board, square, channel) = "
            f"({b}, {p}, {c}): got {float(g[b, p, c])}, expected {float(e[b, p, c])}; " + ("; ".join(notes) or "not confined"))


# ------------------------------------------------------------------------------------------------ (a) the generic kernel
class Geo(NamedTuple):
    dtype: torch.dtype
    Cin: int
    Cout: int
    Cin_real: int = 0
    Cout_real: int = 0
    env: Tuple[Tuple[str, str], ...] = ()

    @property
    def id(self):
        dt = "bf16" if self.dtype == torch.bfloat16 else "f32"
        pad = f"-real{self.Cin_real or self.Cin}x{self.Cout_real or self.Cout}" if (self.Cin_real or self.Cout_real) else ""
        return f"{dt}-{self.Cin}x{self.Cout}{pad}" + "".join(f"-{k[8:]}{v}" for k, v in self.env)


SMALL_B = (1, 2, 3, 5)
BF16_CIN, F32_CIN, COUTS = (32, 96, 160, 192, 256), (16, 48, 256), (16, 48, 80, 144, 272)
bf, f32 = torch.bfloat16, torch.float32
# every Cin against two Cout and every Cout against two Cin: each branch of the chunk choice and each slab shape is reached
GEOMETRY = tuple(dict.fromkeys(
    [Geo(bf, ci, co) for ci in BF16_CIN for co in (48, 272)] + [Geo(bf, ci, co) for ci in (96, 256) for co in COUTS] +
    [Geo(f32, ci, co) for ci in F32_CIN for co in (48, 272)] + [Geo(f32, ci, co) for ci in (48, 256) for co in COUTS]))
# the switches of the generic kernel: tiles per wave, chunk width, two boards per workgroup (odd B: the last one half empty)
TUNED = tuple(Geo(dt, 256, 256, env=env) for dt in (bf, f32) for env in (
    (("KA_CONV_NTW", "1"),), (("KA_CONV_NTW", "2"),), (("KA_CONV_NTW", "4"),), (("KA_CONV_KC", "64"),), (("KA_CONV_KC", "32"),),
    (("KA_CONV_WM", "2"),), (("KA_CONV_WM", "2"), ("KA_CONV_NTW", "4")))) + (Geo(bf, 96, 80, env=(("KA_CONV_WM", "2"),)),)
# padded packs: Co < Nout, and Ci < Kin with data in the padded input channels (the stem's 50 -> 64)
PADDED = (Geo(bf, 64, 64, 50, 64), Geo(f32, 64, 64, 50, 64), Geo(bf, 64, 48, 50, 40), Geo(f32, 32, 80, 17, 70), Geo(bf, 96, 144, 96, 130))
# an ODD number of 16-channel tiles at the batch from which conv_dispatch would keep two (Cout 80) or four (Cout 144) tiles per
# wave: the last tile has no partner to share a 16-byte store with
B_ODD_TILES = 256
ODD_TILES = (Geo(bf, 32, 80), Geo(bf, 32, 144))
PACK_MULTI = (Geo(bf, 64, 48, 50, 40), Geo(f32, 32, 80, 17, 70), Geo(bf, 96, 144), Geo(f32, 48, 272))


def geo_fwd(geo: Geo, transform="plain", adjoint=False) -> Fwd:
    return fwd_data(B_SMALL, geo.Cin, geo.Cout, transform, 2, 3, geo.Cin_real, geo.Cout_real, adjoint)


def geo_dgrad(geo: Geo) -> Dgrad:
    return dgrad_data(B_SMALL, geo.Cin, geo.Cout)


# ------------------------------------------------------------------------------------------------ (b) the training routes
class Form(NamedTuple):
    """A route of conv_dispatch at B >= 512.  env: its switches (all others unset).  routes: ABI entry -> the counters a call must
    raise by one (no other may move); an entry that is absent is not run on the form.  Entries: fwd (plain input), fwdt (scale,
    shift, ReLU and per-board bias), keep (fwdt through ka_conv3x3_fwd_keep with x_out), two (ka_conv3x3_dgrad_fused, plain
    epilogue), masked, gated (ka_conv3x3_dgrad_fused_gated)."""
    name: str
    C: int
    env: dict
    routes: dict
    batches: Tuple[int, ...] = (512, 513, 515)


IN, OUT, PC, GEN = ("pc2_corner_in",), ("pc2_corner_out", "corner"), ("pc", "corner"), ("conv", "corner")
ALL = ("fwd", "fwdt", "keep", "two", "masked", "gated")


def same(routes, *entries):
    return {e: routes for e in entries}


FORMS = (
    # conv3x3_pc2_kernel, 256 channels.  The masked epilogue always leaves square 80 to the corner launch.
    Form("pc2", 256, {}, {**same(IN, "fwd", "fwdt", "keep", "two"), **same(OUT, "masked", "gated")}, (512, 513, 515, 1027)),
    Form("pc2-corner-launch", 256, {"KA_CONV_CORNER_IN": "0"}, same(OUT, *ALL)),
    Form("pc2-stag", 256, {"KA_CONV_PC2_STAG": "1"}, same(OUT, *ALL)),
    Form("pc2-skip", 256, {"KA_CONV_PC2_SKIP": "1"}, same(OUT, *ALL)),
    # conv3x3_pc2_kernel, 128 channels: all 81 squares, no corner, no x_out
    Form("pc2-128", 128, {}, same(("pc2",), "fwd", "fwdt", "two", "masked", "gated")),
    # conv3x3_pc_kernel (KA_CONV_PC2=0): four staging waves for the plain input, two for a transformed one; the two-tensor
    # forms go to conv3x3_kernel<.., 5> unless KA_CONV_P says otherwise
    Form("pc", 256, {"KA_CONV_PC2": "0"}, {**same(PC, "fwd", "fwdt"), **same(GEN, "two", "masked")}),
    Form("pc-npw2", 256, {"KA_CONV_PC2": "0", "KA_CONV_P_NPW": "2"}, same(PC, "fwd", "fwdt")),
    Form("pc-npw4", 256, {"KA_CONV_PC2": "0", "KA_CONV_P_NPW": "4"}, same(PC, "fwd", "fwdt")),
    Form("pc-p3", 256, {"KA_CONV_PC2": "0", "KA_CONV_P": "3"}, same(PC, "fwd", "fwdt", "two", "masked"), (512, 513, 515, 1027)),
    Form("pc-stag", 256, {"KA_CONV_PC2": "0", "KA_CONV_P": "3", "KA_CONV_P_STAG": "1"}, same(PC, "fwd", "fwdt", "two", "masked")),
    Form("pc-mt6", 256, {"KA_CONV_PC2": "0", "KA_CONV_P": "3", "KA_CONV_MT": "6"}, same(("pc",), "fwd", "fwdt", "two", "masked")),
    Form("pc-wgs64", 256, {"KA_CONV_PC2": "0", "KA_CONV_P": "3", "KA_CONV_P_WGS": "64"}, same(PC, "fwd", "fwdt", "two", "masked")),
    # conv3x3_kernel at training batches (KA_CONV_P=0): five row tiles and the corner launch, or all six
    Form("generic", 256, {"KA_CONV_P": "0"}, same(GEN, "fwd", "fwdt", "two", "masked")),
    Form("generic-mt6", 256, {"KA_CONV_P": "0", "KA_CONV_MT": "6"}, same(("conv",), "fwd", "fwdt", "two", "masked")),
)
FORM_CASES = tuple((f, B) for f in FORMS for B in f.batches)

TRAIN_DENSITY = {"fwd": (2, 3), "fwdt": (1, 3)}       # weight density of the forward cases (the issue's measurements)


def train_fwd(C, entry, B=0) -> Fwd:
    num, den = TRAIN_DENSITY[entry]
    return take(fwd_data(B_TRAIN[C], C, C, "plain" if entry == "fwd" else "all", num, den), B or B_TRAIN[C])


def train_dgrad(C, gated, B=0) -> Dgrad:
    """Two-tensor data gradient: weights of density 1/4 (plain; |dy| <= 3) and 1/8 (gated; |dy| <= 5) keep max |dh| <= 256."""
    return take(dgrad_data(B_TRAIN[C], C, C, gated, 1, 8 if gated else 4), B or B_TRAIN[C])


# ------------------------------------------------------------------------------------------------ (c) rounding
B_ROUND = 515


def round_fwd(B=B_ROUND) -> Fwd:
    """x in -2 .. 2, ternary weights of density 2/3, 256 channels: outputs pass 256, where odd integers are ties of bf16."""
    return take(fwd_data(B_ROUND, 256, 256, "plain", 2, 3, xlim=2), B)


def round_dgrad(B=B_ROUND) -> Dgrad:
    return take(dgrad_data(B_ROUND, 256, 256, False, 2, 3, alim=2), B)


def all_case_builders():
    """Every (label, thunk) whose construction asserts the exactness conditions: the CPU test runs them all."""
    out = []
    for geo in GEOMETRY + TUNED + PADDED:
        out.append((f"fwd {geo.id}", lambda geo=geo: geo_fwd(geo)))
        out.append((f"adjoint {geo.id}", lambda geo=geo: geo_fwd(geo, adjoint=True)))
        if geo.dtype == torch.bfloat16 and not (geo.Cin_real or geo.Cout_real):
            out.append((f"dgrad {geo.id}", lambda geo=geo: geo_dgrad(geo)))
    for geo in ODD_TILES:
        out.append((f"odd tiles fwd {geo.id}", lambda geo=geo: fwd_data(B_ODD_TILES, geo.Cin, geo.Cout)))
        out.append((f"odd tiles dgrad {geo.id}", lambda geo=geo: dgrad_data(B_ODD_TILES, geo.Cin, geo.Cout)))
    for tr in TRANSFORMS:
        out.append((f"transform {tr}",lambda tr=tr: fwd_data(B_SMALL, 96, 80, tr)))
        out.append((f"transform {tr} f32", lambda tr=tr: fwd_data(B_SMALL, 48, 80, tr)))
    for C in (256, 128):
        for entry in TRAIN_DENSITY:
            out.append((f"train {entry} {C}", lambda C=C, entry=entry: train_fwd(C, entry)))
        for gated in (False, True):
            out.append((f"train dgrad {C} gated={gated}", lambda C=C, gated=gated: train_dgrad(C, gated)))
    out.append(("round fwd", round_fwd))
    out.append(("round dgrad", round_dgrad))
    return out


# ------------------------------------------------------------------------------------------------ (d) Gaussian data
def gaussian_case(B, C, seed):
    """bf16-rounded N(0, 1) activations and N(0, 1) / (3 sqrt C) weights (held as float32).  The two-tensor coefficients are
    powers of two and k1 = 0, so that dy = a * k0 + in2 * k2 is ONE rounding of an exactly known sum: a * k0 and in2 * k2 are exact,
    and the sum of two bf16 numbers either fits fp32 (exponents within 16) or is the larger one far from any tie -- the kernel's
    fp32 fma followed by the bf16 conversion and the fp64 sum followed by the bf16 conversion give the same bf16."""
    g = gen(4, B, C, seed)
    rb = lambda t: t.to(torch.bfloat16).float()
    x, in2 = rb(torch.randn(B, BOARD, C, generator=g)), rb(torch.randn(B, BOARD, C, generator=g))
    w = rb(torch.randn(C, C, 3, 3, generator=g) / (3 * C ** 0.5))
    k = torch.cat([pick(g, (-2.0, -1.0, -0.5, 0.5, 1.0, 2.0), C), torch.zeros(C), pick(g, (-1.0, -0.5, 0.5, 1.0), C)])
    dy = (x.double() * k[:C].double() + in2.double() * k[2 * C:].double()).to(torch.bfloat16).float()
    return x, in2, w, k, dy


def seq_f32_error(h, w, adjoint, ref, boards=16):
    """max |acc - ref| over the first `boards` boards of a float32 accumulation of the same products ONE AT A TIME, tap by tap and
    channel by channel: the error of the plainest fp32 evaluation (products of bf16-valued operands are exact in fp32, so this is
    the rounding of the 9 Cin additions alone)."""
    n = min(boards, h.shape[0])
    Cin = h.shape[2]
    Cout = w.shape[1] if adjoint else w.shape[0]
    img = torch.zeros(n, 11, 11, Cin)
    img[:, 1:10, 1:10] = h[:n].float().reshape(n, 9, 9, Cin)
    acc = torch.zeros(n, 9, 9, Cout)
    wf = w.float()
    for tap in range(9):
        patch = img[:, tap // 3:tap // 3 + 9, tap % 3:tap % 3 + 9]
        src = 8 - tap
        wt = wf[:, :, src // 3, src % 3] if adjoint else wf[:, :, tap // 3, tap % 3].t()       # (Cin, Cout)
        for c in range(Cin):
            acc += patch[..., c:c + 1] * wt[c]
    return float((acc.double().reshape(n, BOARD, Cout) - ref[:n].double()).abs().max())
