"""The integer oracle of tests/test_hip_wgrad_exact.py, proved on the CPU: the fp64 reference equals torch's own weight
gradient bit for bit (in fp32 too: the sums are exact in any order), the split plan restates the library's, and the comparison
has teeth -- a reference with one of the mistakes a weight-gradient kernel can make fails torch.equal on every case the
mistake applies to."""
import pytest
import torch

from wgrad_helpers import (BOARD, GEOMETRY_CASES, GEOMETRY_SHAPES, INT_CASES, RANGE_CASES, RANGE_TABLE, TRANSFORMS, case_data,
                           ranges_of, ref64, split_plan, tiles, transform64, unfold64)

IDS = [c.id for c in INT_CASES]


def nchw(t):
    B, _, C = t.shape
    return t.reshape(B, 9, 9, C).permute(0, 3, 1, 2).contiguous()


@pytest.mark.parametrize("case", INT_CASES, ids=IDS)
def test_reference_equals_torch_weight_gradient_bit_for_bit(case):
    op, ref = case_data(case)
    h = transform64(op.x, op.scale, op.shift, op.relu, op.bias)
    assert float(h.abs().max()) <= 8 and torch.equal(h, h.to(torch.bfloat16).double()), "h must be exact in bf16"
    shape = (case.Cout, case.Cin, 3, 3)
    for dt in (torch.float64, torch.float32):
        got = torch.nn.grad.conv2d_weight(nchw(h).to(dt), shape, nchw(op.dy).to(dt), padding=1)
        assert torch.equal(got.double(), ref), dt
    assert float(ref.abs().max()) < 2 ** 20
    # (relu without a bias: a channel with scale * x + shift <= 0 for every x in -2..2 is dead, about one in ten)
    dead_ok = TRANSFORMS[case.transform][1] and not TRANSFORMS[case.transform][2]
    assert float((ref != 0).double().mean()) > (0.85 if dead_ok else 0.95), "a dW of zeros would hide a dropped product"


def test_split_plan_reproduces_the_case_tables():
    for B, wgs, lengths in RANGE_TABLE:
        nsplit, bps, got = split_plan(B, 64, 64, wgs)
        assert (nsplit, tuple(got)) == (len(lengths), lengths) and bps == max(lengths), (B, wgs)
    for ci, _, co in GEOMETRY_SHAPES:
        assert split_plan(8, ci, co, 2 * tiles(ci, co)) == (2, 4, [4, 4]), (ci, co)
    assert [tiles(ci, co) for ci, _, co in GEOMETRY_SHAPES] == [1, 1, 2, 2, 6, 3, 8, 2, 1]
    assert split_plan(8, 80, 144, 8) == (2, 4, [4, 4])
    assert split_plan(35, 64, 64, 1) == (1, 35, [35]) and split_plan(40, 256, 256, 16) == (2, 20, [20, 20])
    assert split_plan(4096, 256, 256, 0) == (32, 128, [128] * 32)
    assert split_plan(4096, 256, 256, 192) == (24, 171, [171] * 23 + [163])
    for case in INT_CASES:
        assert tuple(case.plan[2]) == case.lengths and sum(case.lengths) == case.B, case.id


# ------------------------------------------------------------------------------------------------ mutants of the reference
def grad_of(h, dy):
    B, _, Cin = h.shape
    return (dy.double().reshape(B * BOARD, -1).t() @ unfold64(h)).reshape(-1, Cin, 3, 3)


def no_halo(case, op):
    """X tile without the left / right halo: a tap that leaves a board row lands in the neighbouring row."""
    h = transform64(*op[:1], *op[2:])
    B, _, Cin = h.shape
    flat = torch.zeros(B, BOARD + 20, Cin, dtype=torch.float64)
    flat[:, 10:10 + BOARD] = h
    cols = torch.stack([flat[:, 10 + off:10 + off + BOARD] for off in (9 * dr + dc for dr in (-1, 0, 1) for dc in (-1, 0, 1))], dim=3)
    return (op.dy.double().reshape(B * BOARD, -1).t() @ cols.reshape(B * BOARD, Cin * 9)).reshape(-1, Cin, 3, 3)


def last_row_dropped(case, op):
    """The last flat row of every board range never multiplied."""
    dy = op.dy.clone()
    for _, end in ranges_of(case.plan):
        dy[end - 1, BOARD - 1] = 0
    return ref64(op.x, dy, *op[2:])


def row_counted_twice(case, op):
    """Row 80 of the third board of every range of three boards or more multiplied twice."""
    dy = op.dy.clone()
    for beg, end in ranges_of(case.plan):
        if end - beg >= 3:
            dy[beg + 2, BOARD - 1] *= 2
    return ref64(op.x, dy, *op[2:])


def bias_of_previous_board(case, op):
    return ref64(op.x, op.dy, op.scale, op.shift, op.relu, op.bias.roll(1, 0))


def relu_after_bias(case, op):
    h = op.x.double()
    if op.scale is not None:
        h = h * op.scale.double() + op.shift.double()
    return grad_of(torch.relu(h + op.bias.double()[:, None, :]), op.dy)


def padded_channel_folded(case, op):
    """Padded input channel Cin_real added into channel Cin_real - 1."""
    dw = case_data(case)[1].clone()
    dw[:, case.Cin_real - 1] += dw[:, case.Cin_real]
    return dw


MUTANTS = {
    "no_halo": (no_halo, lambda c: True),
    "last_row_dropped": (last_row_dropped, lambda c: True),
    "row_counted_twice": (row_counted_twice, lambda c: max(c.lengths) >= 3),
    "bias_of_previous_board": (bias_of_previous_board, lambda c: TRANSFORMS[c.transform][2] and c.B >= 2),
    "relu_after_bias": (relu_after_bias, lambda c: TRANSFORMS[c.transform][1] and TRANSFORMS[c.transform][2]),
    "padded_channel_folded": (padded_channel_folded, lambda c: c.Cin_real < c.Cin),
}


@pytest.mark.parametrize("name", MUTANTS)
def test_mutant_of_the_reference_fails_on_every_case(name):
    mutant, applies = MUTANTS[name]
    cases = [c for c in INT_CASES if applies(c)]
    assert len(cases) >= 4, "the mutant must meet the range, geometry and transform lists"
    for case in cases:
        op, ref = case_data(case)
        got = mutant(case, op)[:, :case.Cin_real]
        assert got.shape == ref[:, :case.Cin_real].shape
        assert not torch.equal(got, ref[:, :case.Cin_real]), f"{name} passes on {case.id}"


def test_mutant_lists_cover_the_axes():
    """Each axis of the GPU test has a mutant that only it can catch: ranges of three boards, padded channels, the transform."""
    assert sum(max(c.lengths) >= 3 for c in RANGE_CASES) >= 10
    assert sum(c.Cin_real < c.Cin for c in GEOMETRY_CASES) == 4
    assert all(float(case_data(c)[0].x[:, :, c.Cin_real:].abs().max()) > 0 for c in GEOMETRY_CASES if c.Cin_real < c.Cin)
