"""Shared by tests/test_wgrad_exact_cpu.py and tests/test_hip_wgrad_exact.py: integer-valued operands of the 3x3 weight
gradient, its fp64 reference, a restatement of the library's split-K plan, the kernel forms with the switches and the route
counter of each, and the case lists.

Why integers: with x, dy in -2..2, scale in {-2, -1, 1, 2}, shift and per-board bias in -2..2 the transformed input
h = relu(x * scale + shift) + bias is an integer of magnitude <= 8 (exact in bf16), every product dy * h is exact, and every
partial sum is an integer below 2^20 < 2^24: fp32 addition of such numbers is exact in ANY order, so dW must equal the
reference to the bit whatever the MFMA grouping, the k-step walk or the split-K reduce order, and one misplaced product (one
square of one board) changes it."""
import functools
from typing import NamedTuple, Optional, Tuple

import torch

BOARD = 81
TILE_N, TILE_C = 128, 64                         # the output tile the split plan counts (csrc/wgrad.hip: wgrad_splits_for)

# name -> (scale + shift, relu, per-board bias): every combination the ABI admits (scale and shift come together)
TRANSFORMS = {
    "plain": (False, False, False),
    "affine": (True, False, False),
    "relu": (False, True, False),
    "bias": (False, False, True),
    "affine_relu": (True, True, False),
    "relu_bias": (False, True, True),
    "all": (True, True, True),
}

# The kernel forms.  env: the KA_* switches the form needs (every other switch of SWITCHES unset); route: the counter of
# ROUTES (ka_conv_route_counts) a call must raise by one while the other one stays.
SWITCHES = ("KA_WGRAD_LEAN", "KA_WGRAD_TN", "KA_WGRAD_STAG", "KA_WGRAD_WGS")
ROUTES = ("conv", "pc", "pc2", "pc2_corner_in", "pc2_corner_out", "corner", "wgrad_lean", "wgrad_tiled")


class Form(NamedTuple):
    name: str
    dtype: torch.dtype
    env: dict
    route: str


FORMS = (
    Form("bf16-lean", torch.bfloat16, {}, "wgrad_lean"),
    Form("bf16-tiled", torch.bfloat16, {"KA_WGRAD_LEAN": "0"}, "wgrad_tiled"),
    Form("bf16-tn64", torch.bfloat16, {"KA_WGRAD_TN": "64"}, "wgrad_tiled"),
    Form("bf16-lean-nostag", torch.bfloat16, {"KA_WGRAD_STAG": "0"}, "wgrad_lean"),
    Form("bf16-tiled-nostag", torch.bfloat16, {"KA_WGRAD_STAG": "0", "KA_WGRAD_LEAN": "0"}, "wgrad_tiled"),
    Form("f32", torch.float32, {}, "wgrad_tiled"),
    Form("f32-tn64", torch.float32, {"KA_WGRAD_TN": "64"}, "wgrad_tiled"),
)


# ------------------------------------------------------------------------------------------------ operands and reference
class Operands(NamedTuple):
    x: torch.Tensor                              # (B, 81, Cin) float32, integer-valued; so are all the others
    dy: torch.Tensor                             # (B, 81, Cout)
    scale: Optional[torch.Tensor]                # (Cin,) or None
    shift: Optional[torch.Tensor]                # (Cin,) or None
    relu: bool
    bias: Optional[torch.Tensor]                 # (B, Cin) or None


def transform64(x, scale, shift, relu, bias):
    """h = relu(x * scale + shift) + bias in fp64, each step optional: (B, 81, Cin)."""
    h = x.double()
    if scale is not None:
        h = h * scale.double() + shift.double()
    if relu:
        h = torch.relu(h)
    if bias is not None:
        h = h + bias.double()[:, None, :]
    return h


def int_case(seed, B, Cin, Cout, transform) -> Operands:
    """Integer operands (see the module docstring); all Cin channels -- padded ones included -- hold nonzero values."""
    affine, relu, with_bias = TRANSFORMS[transform]
    g = torch.Generator().manual_seed(seed)
    small = lambda *s: torch.randint(-2, 3, s, generator=g).float()
    x, dy = small(B, BOARD, Cin), small(B, BOARD, Cout)
    scale = torch.tensor([-2.0, -1.0, 1.0, 2.0])[torch.randint(0, 4, (Cin,), generator=g)]
    shift, bias = small(Cin), small(B, Cin)
    op = Operands(x, dy, scale if affine else None, shift if affine else None, relu, bias if with_bias else None)
    h = transform64(op.x, op.scale, op.shift, op.relu, op.bias)
    assert BOARD * B * float(dy.abs().max()) * float(h.abs().max()) < 2 ** 20, "partial sums must stay exact in fp32"
    return op


def unfold64(h):
    """(B, 81, Cin) -> (B * 81, Cin * 9) fp64: row (b, p) holds h[b, p + tap, c] at column c * 9 + tap, zero outside the board."""
    B, _, Cin = h.shape
    cols = torch.nn.functional.unfold(h.double().reshape(B, 9, 9, Cin).permute(0, 3, 1, 2), 3, padding=1)   # (B, Cin * 9, 81)
    return cols.transpose(1, 2).reshape(B * BOARD, Cin * 9)


def ref64(x, dy, scale=None, shift=None, relu=False, bias=None):
    """dW (Cout, Cin, 3, 3) fp64 = dy^T unfold(h)."""
    B, _, Cin = x.shape
    Cout = dy.shape[2]
    h = transform64(x, scale, shift, relu, bias)
    return (dy.double().reshape(B * BOARD, Cout).t() @ unfold64(h)).reshape(Cout, Cin, 3, 3)


def seq_f32_error(x, dy, ref):
    """max |acc - ref| of a float32 accumulation of the 81 * B row outer products dy[row]^T unfold(x)[row], one row at a time
    in flat order: the error of the plainest fp32 evaluation of the same sum (the products of bf16-valued operands are exact
    in fp32, so this is rounding of the additions alone)."""
    B, _, Cin = x.shape
    Cout = dy.shape[2]
    cols, rows = unfold64(x).float(), dy.float().reshape(B * BOARD, Cout)
    acc = torch.zeros(Cout, Cin * 9)
    for k in range(B * BOARD):
        acc += torch.outer(rows[k], cols[k])
    return float((acc.double().reshape(Cout, Cin, 3, 3) - ref).abs().max())


# ------------------------------------------------------------------------------------------------ the split-K plan
def tiles(Cin, Cout):
    return -(-Cout // TILE_N) * -(-Cin // TILE_C)


def split_plan(B, Cin, Cout, target_wgs):
    """(nsplit, boards_per_split, [range lengths]): wgrad_splits_for of csrc/wgrad.hip restated (target_wgs 0 = 256)."""
    s = max(1, min(B, (target_wgs if target_wgs > 0 else 256) // tiles(Cin, Cout)))
    bps = -(-B // s)
    nsplit = -(-B // bps)
    return nsplit, bps, [min(bps, B - i * bps) for i in range(nsplit)]


def ranges_of(plan):
    """[(first board, one past the last board)] of a split plan."""
    out, b = [], 0
    for n in plan[2]:
        out.append((b, b + n))
        b += n
    return out


# ------------------------------------------------------------------------------------------------ the cases
class Case(NamedTuple):
    B: int
    Cin: int
    Cin_real: int
    Cout: int
    target_wgs: int
    transform: str
    lengths: Tuple[int, ...]                     # the range lengths the case claims to reach

    @property
    def id(self):
        return f"B{self.B}-{self.Cin}.{self.Cin_real}x{self.Cout}-wgs{self.target_wgs}-{self.transform}"

    @property
    def plan(self):
        return split_plan(self.B, self.Cin, self.Cout, self.target_wgs)


# (a) range lengths at one 64 x 64 tile: B, target_wgs, ranges
RANGE_TABLE = (
    (9, 0, (1,) * 9),                            # one board per split: the regime of the older tests
    (1, 1, (1,)), (2, 1, (2,)), (3, 1, (3,)), (4, 1, (4,)),      # ring not entered, half, full, first wrap
    (7, 3, (3, 3, 1)),                           # short last split, 5 padding workgroups
    (11, 4, (3, 3, 3, 2)),
    (19, 10, (2,) * 9 + (1,)),                   # nsplit > 8: second slot group of the XCD map
    (32, 1, (32,)),                              # 2592 rows = 81 whole steps, no pad rows in the last step
    (33, 1, (33,)),                              # one board past the 32-board phase period of 81 j mod 32
    (35, 1, (35,)),                              # 88 steps and a 19-row tail
    (70, 2, (35, 35)),
)
RANGE_CASES = tuple(Case(B, 64, 64, 64, wgs, tr, ln) for B, wgs, ln in RANGE_TABLE for tr in ("plain", "all"))

# (b) channel geometry at two ranges of four boards: Cin, Cin_real, Cout
GEOMETRY_SHAPES = ((16, 16, 16), (48, 48, 80), (64, 64, 144), (80, 80, 128), (96, 96, 272), (144, 144, 64), (256, 256, 256),
                   (64, 50, 256), (32, 17, 48))
GEOMETRY_CASES = tuple(Case(8, ci, cr, co, 2 * tiles(ci, co), tr, (4, 4)) for ci, cr, co in GEOMETRY_SHAPES for tr in ("plain", "all"))

# (c) every transform combination
TRANSFORM_CASES = tuple(Case(8, 80, 80, 144, 8, tr, (4, 4)) for tr in TRANSFORMS)

INT_CASES = RANGE_CASES + GEOMETRY_CASES + TRANSFORM_CASES


@functools.lru_cache(maxsize=None)
def case_data(case: Case):
    """(operands, fp64 reference over all Cin channels) of a case, computed once; neither may be modified."""
    seed = 7919 * case.B + 31 * case.Cin + case.Cout + 1000003 * list(TRANSFORMS).index(case.transform)
    op = int_case(seed, case.B, case.Cin, case.Cout, case.transform)
    return op, ref64(*op)


def accumulate_pattern(case: Case):
    """Integers in -3..3 in the shape of dW: what dW holds before an accumulating call."""
    g = torch.Generator().manual_seed(case.Cin_real * 1009 + case.Cout)
    return torch.randint(-3, 4, (case.Cout, case.Cin_real, 3, 3), generator=g).float()
